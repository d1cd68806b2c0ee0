"""Thin torch-facing wrappers over the C ABI (one call = one asynchronous launch on the
current torch stream).  Tensors are passed as raw device pointers; nothing here computes."""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib

EPSILON = 1e-7  # keras epsilon, bear_model/core.py:8


class _Handle:
    """Owner of one handle of the library: ``_create`` fills ``_h`` through the out-parameter that the create entry ``name`` takes
    behind ``args`` (and, when given, ahead of ``after``); the entry ``_destroy`` names releases it with the object."""
    _destroy = None

    def _create(self, name, *args, after=()):
        h = ctypes.c_void_p()
        _lib.call(name, *args, ctypes.byref(h), *after)
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                getattr(_lib.lib(), self._destroy)(h)
            except Exception:
                pass


class Workspace(_Handle):
    """Owns a bear_ws handle for one device (per-block partial sums)."""
    _destroy = "bear_ws_destroy"

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("bear_amd requires an MI355X (HIP) device; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        self._create("bear_ws_create", self.device.index)

    @property
    def handle(self):
        return self._h


_default_ws = {}


def default_workspace(device, for_capture=False):
    """The workspace of (device, current stream).  A workspace serves ONE stream at a time (include/bear_hip.h: its block
    partials and the arrival counter of the "last block finalizes" kernels are per-launch state), so a side stream gets its own;
    a stream that is capturing a graph shares the device's first workspace (nothing may be allocated during capture, and a
    capture orders every launch of the step on that one stream anyway)."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    stream = torch.cuda.current_stream(idx)
    key = (idx, 0 if (for_capture or stream == torch.cuda.default_stream(idx) or torch.cuda.is_current_stream_capturing())
           else stream.cuda_stream)       # for_capture: the one a capturing stream will resolve to (created BEFORE the capture)
    ws = _default_ws.get(key)
    if ws is None:
        ws = _default_ws[key] = Workspace(torch.device("cuda", idx))
    return ws


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(device, name, *args):
    """The entry point ``name`` with ``device`` current, on the current torch stream (every launching entry's last argument)."""
    with torch.cuda.device(device):
        _lib.call(name, *args, _stream())


WIDE_WIDTHS = (5, 21)   # row widths of the *_wide entry points: the protein alphabet (20 letters + stop), and 5 for cross-checks


def _check_rows(t, dtype, name, width=5, n=None, clone=True):
    """``t`` as the C ABI takes rows: a contiguous CUDA tensor [N, width] (``n``: [n, width]) of ``dtype``, 16-byte aligned.
    ``width`` None: the width ``t`` has, for the *_wide entries; every width is one of ``WIDE_WIDTHS``.  A misaligned ``t`` (a slice
    of such a tensor may start on any row) comes back as a copy; ``clone=False`` refuses it instead -- where the kernel must see
    the caller's own buffer (a plan is tied to it, or the kernel writes it)."""
    if width is None and t.dim() == 2:
        width = t.shape[1]
    if not (t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == width and t.is_contiguous()
            and (n is None or t.shape[0] == n)):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of shape [{'N' if n is None else n}, {width or 'W'}] and dtype {dtype}")
    if width not in WIDE_WIDTHS:
        raise ValueError(f"{name}: rows of width {width}; the kernels take {WIDE_WIDTHS}")
    if t.data_ptr() % 16:
        if not clone:
            raise ValueError(f"{name} must be 16-byte aligned")
        t = t.clone()
    return t


def counts_dtype():
    """Counts travel as 32-bit words (KMC's counter range, summarize.py:66-67). torch has no
    general uint32 arithmetic, so int32 storage is used and reinterpreted by the kernel."""
    return torch.int32


def dm_prior(counts, prior, h_signed, eps=EPSILON, train_ar=False, want_grad=False, out=None, ws=None):
    """sum LL and d/dh_signed over rows (bear_net._train_step arithmetic, bear_net.py:146-197).
    Returns (out[2] device tensor, grad_prior or None)."""
    counts = _check_rows(counts, torch.int32, "counts")
    prior = _check_rows(prior, torch.float64, "prior")
    if counts.shape[0] != prior.shape[0]:
        raise ValueError("counts and prior must have the same number of rows")
    ws = ws or default_workspace(counts.device)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    grad = torch.empty_like(prior) if want_grad else None
    _launch(counts.device, "bear_dm_prior_f64", ws.handle, _ptr(counts), _ptr(prior), counts.shape[0], float(h_signed), float(eps),
            int(bool(train_ar)), _ptr(out), _ptr(grad))
    return out, grad


def dm_prior_wide(counts, prior, h_signed_dev, eps=EPSILON, train_ar=False, want_grad=False, out=None, ws=None):
    """``bear_dm_prior_wide_f64``: ``dm_prior`` for rows of width W = ``counts.shape[-1]`` (21: the protein alphabet), with h_signed
    read from the device tensor ``h_signed_dev`` [1] (a step is enqueued without a host read-back and can be captured).
    Returns (out[2] device tensor = sum LL, d/dh_signed; grad_prior [N, W] or None)."""
    counts = _check_rows(counts, torch.int32, "counts", None)
    width = counts.shape[1]
    prior = _check_rows(prior, torch.float64, "prior", width)
    if counts.shape[0] != prior.shape[0]:
        raise ValueError("counts and prior must have the same number of rows")
    if h_signed_dev is not None:
        _f64_vec(h_signed_dev, 1, "h_signed_dev")
    elif not train_ar:
        raise ValueError("h_signed_dev is needed in BEAR mode")
    ws = ws or default_workspace(counts.device)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    grad = torch.empty_like(prior) if want_grad else None
    _launch(counts.device, "bear_dm_prior_wide_f64", ws.handle, _ptr(counts), _ptr(prior), counts.shape[0], width, _ptr(h_signed_dev),
            float(eps), int(bool(train_ar)), _ptr(out), _ptr(grad))
    return out, grad


# tiles and resident blocks per CU of the bear_ref kernels at a wide row (kernels_refmix_wide.h: RFW_TILE / RMW_TILE and
# *_BLOCKS_PER_CU): a launch takes min(tiles, blocks per CU * CUs) blocks -- tests size a table beyond that from these
REF_WIDE_TILE = {21: 256, 5: 512}
REFMIX_WIDE_TILE = {21: 128, 5: 512}
REF_WIDE_BLOCKS_PER_CU = 3
REFMIX_WIDE_BLOCKS_PER_CU = 3


def _check_ref_wide(train, ref):
    train = _check_rows(train, torch.int32, "train", None)
    ref = _check_rows(ref, torch.int32, "ref", train.shape[1])
    if train.shape[0] != ref.shape[0]:
        raise ValueError("train and ref must have the same number of rows")
    return train, ref


def dm_ref_wide(train, ref, h_signed, tau_signed, nu_signed, eps=EPSILON, train_ar=False, out=None, ws=None):
    """``bear_dm_ref_wide_f64``: ``dm_ref`` for rows of width W = ``train.shape[-1]`` (21: the protein alphabet) -- the stop net
    function, the reference mixing inside the DM kernel, no prior rows.  Returns out [4] = sum LL, d/dh_signed, d/dtau_signed,
    d/dnet_weight_signed."""
    train, ref = _check_ref_wide(train, ref)
    ws = ws or default_workspace(train.device)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=train.device)
    _f64_vec(out, 4, "out")
    _launch(train.device, "bear_dm_ref_wide_f64", ws.handle, _ptr(train), _ptr(ref), train.shape[0], train.shape[1], float(h_signed),
            float(tau_signed), float(nu_signed), float(eps), int(bool(train_ar)), _ptr(out))
    return out


def ref_train_reduce_wide(train, ref, theta, packed, eps=EPSILON, train_ar=False, ws=None):
    """Enqueues ``bear_ref_train_reduce_wide_f64``: ``ref_train_reduce`` for rows of 21 (or 5), without a plan -- this shard's
    packed = [sum LL, d/dh_s, d/dtau_s, d/dnu_s], the kernel constants from the device-resident theta."""
    train, ref = _check_ref_wide(train, ref)
    _f64_vec(theta, 3, "theta")
    _f64_vec(packed, 4, "packed")
    ws = ws or default_workspace(train.device)
    _launch(train.device, "bear_ref_train_reduce_wide_f64", ws.handle, _ptr(train), _ptr(ref), train.shape[0], train.shape[1], _ptr(theta),
            float(eps), int(bool(train_ar)), _ptr(packed))


def ref_train_step_wide(train, ref, theta, adam_m, adam_v, adam_t, learning_rate, scale, out, loss_buf=None, eps=EPSILON, train_ar=False,
                        ws=None):
    """Enqueues one ``bear_ref_train_step_wide_f64``: ``ref_train_step`` for rows of 21 (or 5), without a plan -- constants from
    theta, the wide mode-R kernel, its last block's sums and Adam on theta in one launch; capturable in a HIP graph."""
    train, ref = _check_ref_wide(train, ref)
    for t, n, name in ((theta, 3, "theta"), (adam_m, 3, "adam_m"), (adam_v, 3, "adam_v"), (adam_t, 1, "adam_t"), (out, 4, "out")):
        _f64_vec(t, n, name)
    if loss_buf is not None:
        _f64_vec(loss_buf, loss_buf.numel(), "loss_buf")
    ws = ws or default_workspace(train.device)
    _launch(train.device, "bear_ref_train_step_wide_f64", ws.handle, _ptr(train), _ptr(ref), train.shape[0], train.shape[1], _ptr(theta),
            _ptr(adam_m), _ptr(adam_v), _ptr(adam_t), float(eps), int(bool(train_ar)), float(learning_rate), float(scale), _ptr(out),
            *_loss(loss_buf))


def dm_refmix_wide_dev(counts, net_rows, ref, h_signed_dev, tau_signed_dev, net_weight_signed_dev, eps=EPSILON, out=None, train_ar=False,
                       ws=None):
    """``bear_dm_refmix_wide_grad_f64``: bear_ref's step for a net function with parameters on rows of width W =
    ``counts.shape[-1]`` -- the reference mixing inside the DM kernel.  ``ref`` are the reference COUNTS (int32 storage, as
    ``counts``), ``net_rows`` [n, W] the net function's rows (any non-negative rows: not assumed normalised).
    Returns (out [4] = sum LL, d/dh_signed, d/dtau_signed, d/dnet_weight_signed; d sum LL / d net_rows [n, W])."""
    counts, ref = _check_ref_wide(counts, ref)
    net_rows = _check_rows(net_rows, torch.float64, "net_rows", counts.shape[1])
    if net_rows.shape[0] != counts.shape[0]:
        raise ValueError("counts and net_rows must have the same number of rows")
    _check_scalar_param(h_signed_dev=h_signed_dev, tau_signed_dev=tau_signed_dev, net_weight_signed_dev=net_weight_signed_dev)
    ws = ws or default_workspace(counts.device)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=counts.device)
    _f64_vec(out, 4, "out")
    grad = torch.empty_like(net_rows)
    _launch(counts.device, "bear_dm_refmix_wide_grad_f64", ws.handle, _ptr(counts), _ptr(net_rows), _ptr(ref), counts.shape[0],
            counts.shape[1], _ptr(h_signed_dev), _ptr(tau_signed_dev), _ptr(net_weight_signed_dev), float(eps), int(bool(train_ar)),
            _ptr(out), _ptr(grad))
    return out, grad


def dm_ref(train, ref, h_signed, tau_signed, nu_signed, eps=EPSILON, train_ar=False, out=None, ws=None):
    """[sum LL, d/dh_signed, d/dtau_signed, d/dnet_weight_signed] (bear_ref._train_step
    arithmetic with the stop net function, bear_ref.py:207-259)."""
    train = _check_rows(train, torch.int32, "train")
    ref = _check_rows(ref, torch.int32, "ref")
    if train.shape[0] != ref.shape[0]:
        raise ValueError("train and ref must have the same number of rows")
    ws = ws or default_workspace(train.device)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=train.device)
    _launch(train.device, "bear_dm_ref_f64", ws.handle, _ptr(train), _ptr(ref), train.shape[0], float(h_signed), float(tau_signed),
            float(nu_signed), float(eps), int(bool(train_ar)), _ptr(out))
    return out


class Plan(_Handle):
    """Count-dependent part of the hot path for a table that stays resident across optimizer steps
    (work items sorted by count; include/bear_hip.h "Planned variants").  Keeps the count tensor alive.

    Streams: construction waits for the current stream, runs on the default stream and ends in a device-wide wait (a set-up path).
    ``self.ws`` is the workspace it was created with -- the current stream's unless one is given; a STEP on the plan launches with
    the workspace of the stream that is current when it is enqueued (``_step_ws``), so a plan built on one stream may be stepped on
    another.  The convolutional step alone keeps state in ``self.ws`` (its reservation) and is refused on any other stream."""
    _destroy = "bear_plan_destroy"

    def __init__(self, counts, ncol, ws=None, ref=None, rows_if_dense=False):
        """ref (ncol = 4 only): the reference column the planned mode-R entries will be called with -- the plan then folds the
        contexts without reference counts into a histogram (``bear_plan_create_ref``).
        rows_if_dense (ncol = 5, a plan for ``dm_prior_planned`` / ``dm_prior_planned_dev`` ONLY): ``bear_plan_create_auto`` -- a table
        whose cells are mostly beyond the product path gets the dense form (``self.rowwise``: nothing kept per item, the step streams
        the count and prior rows); the fused linear / convolutional steps refuse such a plan."""
        counts = _check_rows(counts, torch.int32, "counts")
        self.counts = counts
        self.ncol = int(ncol)
        self.ref = None
        self.rowwise = False
        self.ws = ws or default_workspace(counts.device)
        with torch.cuda.device(counts.device):
            torch.cuda.current_stream().synchronize()  # plan construction runs on the default stream
            if ref is not None:
                if self.ncol != 4:
                    raise ValueError("a reference-aware plan needs ncol = 4")
                self.ref = ref = _check_rows(ref, torch.int32, "ref", n=counts.shape[0], clone=False)
                self._create("bear_plan_create_ref", self.ws.handle, _ptr(counts), _ptr(ref), counts.shape[0])
            elif rows_if_dense:
                if self.ncol != 5:
                    raise ValueError("rows_if_dense: five-column plans")
                rw = ctypes.c_int(0)
                self._create("bear_plan_create_auto", self.ws.handle, _ptr(counts), counts.shape[0], ctypes.byref(rw))
                self.rowwise = bool(rw.value)
            else:
                self._create("bear_plan_create", self.ws.handle, _ptr(counts), counts.shape[0], self.ncol)

    @property
    def nbytes(self):
        return int(_lib.lib().bear_plan_bytes(self._h))

    def _optional(self, name, *args):
        """The set-up entry ``name`` of this plan, an optional speed-up that allocates with hipMalloc: out of memory, it is tried
        once more with the torch allocator's cached slabs given back (they are out of hipMalloc's reach).  Given back only then --
        emptying the cache on every call made a streamed epoch pay hipFree / hipMalloc (device-wide synchronisations that serialise
        with the side stream's prefetch) on every batch load.  False when it still ran out: the caller goes without."""
        with torch.cuda.device(self.counts.device):
            st = getattr(_lib.lib(), name)(self._h, *args, _stream())
            if st == _lib.ERR_NOMEM:
                torch.cuda.empty_cache()
                st = getattr(_lib.lib(), name)(self._h, *args, _stream())
        if st != _lib.ERR_NOMEM:
            _lib.check(st, name)
        return st == 0

    def pair_contexts(self, kmer_index, lag):
        """``bear_plan_pair_contexts``: ties this (five-column) plan to the index words ``kmer_index`` (``linear_index``) of its rows
        so that the fused linear step takes neighbouring contexts with equal leading letters two at a time.  Returns False when the
        table is too sparse for it (the plan is then unchanged).  The tensor is kept alive; it must not be modified afterwards."""
        _check_codes(kmer_index)
        if kmer_index.shape[0] != self.counts.shape[0] or kmer_index.data_ptr() % 16:
            raise ValueError("kmer_index: one 16-byte aligned index word per row of the plan's count slab")
        ok = ctypes.c_int(0)
        if not self._optional("bear_plan_pair_contexts", _ptr(kmer_index), int(lag), ctypes.byref(ok)):
            # a table close to the card's capacity runs the plain step
            warnings.warn("bear_plan_pair_contexts: out of device memory, the linear step keeps its plain lists")
            self.paired_codes = None
            return False
        self.paired_codes = kmer_index if ok.value else None
        return bool(ok.value)

    def count_total(self):
        """(total, bound) -- each [sum of all counts, cells that hold a count, largest count]: of the plan's table, and the values in
        force for the deterministic mode's fixed-point scale (``bear_plan_count_total``)."""
        a, b = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
        _lib.call("bear_plan_count_total", self._h, a, b)
        return list(a), list(b)

    def set_count_bound(self, bound):
        """``bear_plan_set_count_bound``: [sum of counts, non-zero cells, largest count] of EVERYTHING that is added into one gradient
        together with this plan's rows (BEAR_AMD_DETERMINISTIC: the scale of the fixed-point gradient tables; ranks that share a batch
        must agree on it: sums of the first two, maximum of the third)."""
        _lib.call("bear_plan_set_count_bound", self._h, (ctypes.c_double * 3)(*[float(x) for x in bound]))

    def pair_info(self):
        """(tiles that take the paired form of the linear step, tiles that keep their plain list) -- ``bear_plan_pair_info``."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.lib().bear_plan_pair_info(self._h, ctypes.byref(a), ctypes.byref(b))
        return int(a.value), int(b.value)

    def attach_cnn_levels(self, kmer_code, lag, filter_width):
        """``bear_plan_attach_cnn_levels``: prefix levels of the (k-mer-sorted) packed contexts ``kmer_code`` (``pack_kmers``) of this
        plan's rows for the convolutional training step -- a position is then evaluated once per distinct prefix.  Returns the
        number of levels attached (0: the step runs as before).  The tensor is kept alive; it must not be modified afterwards."""
        _check_codes(kmer_code)
        if kmer_code.shape[0] != self.counts.shape[0] or kmer_code.data_ptr() % 16:
            raise ValueError("kmer_code: one 16-byte aligned packed context per row of the plan's count slab")
        n = ctypes.c_int(0)
        if not self._optional("bear_plan_attach_cnn_levels", _ptr(kmer_code), int(lag), int(filter_width), ctypes.byref(n)):
            warnings.warn("bear_plan_attach_cnn_levels: out of device memory, the convolutional step runs without prefix levels")
            self.cnn_codes = None
            return 0
        self.cnn_codes = kmer_code if (n.value or self.cnn_window_rows()) else None     # (kept alive: levels and window tables are tied to it)
        return int(n.value)

    def cnn_window_rows(self):
        """[(level, position, distinct windows)] of the window tables attached with the prefix levels (``bear_plan_cnn_window_rows``;
        level 0 = the contexts)."""
        n = int(_lib.lib().bear_plan_cnn_window_rows(self._h, None, None, None, 0))
        if n <= 0:
            return []
        rows, pos, lev = (ctypes.c_uint64 * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
        _lib.lib().bear_plan_cnn_window_rows(self._h, rows, pos, lev, n)
        return [(int(lev[q]), int(pos[q]), int(rows[q])) for q in range(n)]

    def cnn_level_rows(self, with_letters=False):
        """Rows of the attached prefix levels 1 .. n (``bear_plan_cnn_level_rows``); [] without levels.  ``with_letters``: (rows,
        prefix lengths)."""
        n = int(_lib.lib().bear_plan_cnn_level_rows(self._h, None, None, 0))
        if n <= 0:
            return ([], []) if with_letters else []
        rows, letters = (ctypes.c_uint64 * n)(), (ctypes.c_int * n)()
        _lib.lib().bear_plan_cnn_level_rows(self._h, rows, letters, n)
        return ([int(r) for r in rows], [int(x) for x in letters]) if with_letters else [int(r) for r in rows]

    def tiles(self):
        """Diagnostics (``bear_plan_tile_info``): (row0 [T] uint64, rows [T] uint32, items [T] uint32, stream_offset [T] uint64)."""
        n = int(_lib.lib().bear_plan_tile_count(self._h))
        row0, rows, items, off = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint64)
        _lib.call("bear_plan_tile_info", self._h, 0, n, row0.ctypes.data, rows.ctypes.data, items.ctypes.data, off.ctypes.data)
        return row0, rows, items, off


def _step_ws(plan, owns=None):
    """The workspace a step on ``plan`` (a ``Plan`` or an ``EvalPlan``) launches with: the CURRENT stream's (``default_workspace``),
    whichever stream the plan was built on.  A workspace serves one stream at a time (include/bear_hip.h) and a plan binds none
    -- ``ws`` is an argument of every planned entry -- so a plan built on the default stream and stepped on a side stream must not
    take the default stream's block partials and arrival word along (``plan.ws`` is the workspace the plan was CREATED with).
    ``owns``: what of the step lives in ``plan.ws`` itself (the convolutional step's reservation, ``cnn_step_buffers``): such a step
    runs on the stream that owns that workspace and is refused with a ValueError on any other.  A capturing stream resolves to the
    device's first workspace, the default stream's; a workspace handed to the plan explicitly is the caller's to keep to one stream."""
    ws = default_workspace((plan.counts if isinstance(plan, Plan) else plan.test).device)
    if owns is None or ws is plan.ws:
        return ws
    if any(plan.ws is w for w in _default_ws.values()):
        raise ValueError(f"one workspace serves one stream at a time: {owns} lives in the workspace of the stream this plan was built "
                         "on, and the current stream is another one -- build the plan (and reserve) under the stream that steps it")
    return plan.ws


def _check_planned(plan, ncol, rows, dtype, name):
    """``rows``: the caller's aligned buffer with one row per context of a plan of ``ncol`` columns."""
    if plan.ncol != ncol:
        raise ValueError(f"a plan with ncol={ncol} is needed, this one has ncol={plan.ncol}")
    _check_rows(rows, dtype, name, n=plan.counts.shape[0], clone=False)


def dm_prior_planned(plan, prior, h_signed, eps=EPSILON, out=None, normalized=False, want_grad=False, train_ar=False):
    """Planned twin of dm_prior (BEAR mode): [sum LL, d/dh_signed]; with want_grad also the gradient rows
    d sum LL / d prior, returned as (out, grad).  normalized=True asserts that every prior row sums to one
    (any softmax output)."""
    counts = plan.counts
    _check_planned(plan, 5, prior, torch.float64, "prior")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    if want_grad:
        grad = torch.empty_like(prior)
        _launch(counts.device, "bear_dm_prior_plan_grad_f64", _step_ws(plan).handle, plan._h, _ptr(counts), _ptr(prior), counts.shape[0],
                float(h_signed), float(eps), int(bool(train_ar)), int(bool(normalized)), _ptr(out), _ptr(grad))
        return out, grad
    _launch(counts.device, "bear_dm_prior_plan_f64", _step_ws(plan).handle, plan._h, _ptr(counts), _ptr(prior), counts.shape[0], float(h_signed),
            float(eps), int(bool(train_ar)), int(bool(normalized)), _ptr(out))
    return out


def dm_ref_planned(plan, ref, h_signed, tau_signed, nu_signed, eps=EPSILON, out=None, train_ar=False):
    """Planned twin of dm_ref (BEAR mode): [sum LL, d/dh_signed, d/dtau_signed, d/dnet_weight_signed]."""
    train = plan.counts
    _check_planned(plan, 4, ref, torch.int32, "ref")
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=train.device)
    _launch(train.device, "bear_dm_ref_plan_f64", _step_ws(plan).handle, plan._h, _ptr(train), _ptr(ref), train.shape[0], float(h_signed),
            float(tau_signed), float(nu_signed), float(eps), int(bool(train_ar)), _ptr(out))
    return out


def dm_items(x, c, path=0, ws=None):
    """D = lgamma(x+c) - lgamma(x), P = digamma(x+c) - digamma(x) per item (diagnostic entry)."""
    if not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and c.is_cuda and c.dtype == torch.int32
            and c.is_contiguous() and x.shape == c.shape and x.dim() == 1):
        raise ValueError("x: contiguous CUDA float64 [n]; c: contiguous CUDA int32 [n]")
    ws = ws or default_workspace(x.device)
    D, P = torch.empty_like(x), torch.empty_like(x)
    _launch(x.device, "bear_dm_items_f64", ws.handle, _ptr(x), _ptr(c), x.shape[0], int(path), _ptr(D), _ptr(P))
    return D, P


def _probe_ops():
    import re
    text = open(_lib.HEADER_PATH).read()
    return {name.lower(): int(v) for name, v in re.findall(r"^#define BEAR_PROBE_(\w+) (\d+)\s*$", text, flags=re.M) if name != "N_OPS"}


PROBE_OPS = _probe_ops()                                    # name -> op of bear_math_probe_f64, as include/bear_hip.h numbers them
PROBE_ITEM_OPS = ("srt_general", "srt_general_fast", "srt_general_auto", "row_item_tab", "row_item")


def math_probe(op, a, b=None, ws=None):
    """One device math routine, element by element (diagnostic entry; include/bear_hip.h, bear_math_probe_f64): ``op`` a key of
    ``PROBE_OPS``, ``a`` a contiguous CUDA float64 [n].  The item routines (``PROBE_ITEM_OPS``) take the counts ``b`` as float64 [n]
    and return (D, P); every other routine returns one tensor."""
    item = op in PROBE_ITEM_OPS
    if not (a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and a.dim() == 1):
        raise ValueError("a: contiguous CUDA float64 [n]")
    if item != (b is not None) or (item and not (b.is_cuda and b.dtype == torch.float64 and b.is_contiguous() and b.shape == a.shape)):
        raise ValueError("b: contiguous CUDA float64 [n] for the item routines, None otherwise")
    ws = ws or default_workspace(a.device)
    out0 = torch.empty_like(a)
    out1 = torch.empty_like(a) if item else None
    _launch(a.device, "bear_math_probe_f64", ws.handle, int(PROBE_OPS[op]), _ptr(a), _ptr(b), a.shape[0], _ptr(out0), _ptr(out1))
    return (out0, out1) if item else out0


LINEAR_MAX_LAG = 21   # LIN_MAX_LAG of kernels_linear.h (3 bits per letter in one 64-bit word)


def pack_kmers(codes):
    """int8 code matrix [n, lag] (core.encode_kmers) -> packed contexts, int64 storage [n] (3 bits per letter)."""
    if not (codes.is_cuda and codes.dtype == torch.int8 and codes.dim() == 2 and codes.is_contiguous()):
        raise ValueError("codes must be a contiguous CUDA int8 tensor [n, lag]")
    out = torch.empty(codes.shape[0], dtype=torch.int64, device=codes.device)
    _launch(codes.device, "bear_pack_kmers_u64", _ptr(codes), codes.shape[0], codes.shape[1], _ptr(out))
    return out


def linear_index(kmer_code, lag):
    """Packed contexts (``pack_kmers``) -> the table-row words the fused linear head reads (``bear_linear_index_u64``); once per
    batch, the contexts do not change between steps."""
    _check_codes(kmer_code)
    out = torch.empty_like(kmer_code)
    _launch(kmer_code.device, "bear_linear_index_u64", _ptr(kmer_code), kmer_code.shape[0], int(lag), _ptr(out))
    return out


def dm_linear(plan, kmer_index, mat, h_signed, eps=EPSILON, train_ar=False, out=None):
    """One launch of ``bear_dm_linear_f64``: the bear_net step with the linear AR function fused on the plan.
    ``kmer_index`` = ``linear_index(pack_kmers(codes), lag)``.
    Returns (out[2] = {sum LL, d/dh_signed}, grad_mat [lag,5,5] = d sum LL / d mat)."""
    n = plan.counts.shape[0]
    kmer_code = kmer_index
    if not (kmer_code.is_cuda and kmer_code.dtype == torch.int64 and kmer_code.dim() == 1 and kmer_code.is_contiguous()
            and kmer_code.shape[0] == n):
        raise ValueError("kmer_index must be a contiguous CUDA int64 tensor [n_rows] (linear_index)")
    if kmer_code.data_ptr() % 16:
        kmer_code = kmer_code.clone()
    if not (mat.is_cuda and mat.dtype == torch.float64 and mat.dim() == 3 and mat.shape[1:] == (5, 5) and mat.is_contiguous()):
        raise ValueError("mat must be a contiguous CUDA float64 tensor [lag, 5, 5]")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=mat.device)
    grad = torch.empty_like(mat)
    _launch(mat.device, "bear_dm_linear_f64", _step_ws(plan).handle, plan._h, _ptr(plan.counts), _ptr(kmer_code), _ptr(mat), mat.shape[0], n,
            float(h_signed), float(eps), int(bool(train_ar)), _ptr(out), _ptr(grad))
    return out, grad


def _host_f64(values):
    """(array, its address) of host float64 values for a call; None or no values: an empty array and NULL."""
    if values is None or not np.size(values):
        return np.zeros(0), ctypes.c_void_p(0)
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float64)))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _evaluate(wide, test, prior, h, van_reg, train, eps, with_ar, noise_seed, row_base, ws):
    test = _check_rows(test, torch.int32, "test", None if wide else 5)
    n, width = test.shape
    if train is not None:
        train = _check_rows(train, torch.int32, "train", width)
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", width)
    for t in (train, prior):
        if t is not None and t.shape[0] != n:
            raise ValueError("test, train and prior must have the same number of rows")
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(van_reg)
    ws = ws or default_workspace(test.device)
    out = torch.empty(2 * (hs.size + vs.size) + 3, dtype=torch.float64, device=test.device)
    _launch(test.device, "bear_eval_wide_f64" if wide else "bear_eval_f64", ws.handle, _ptr(test), _ptr(train), _ptr(prior), n,
            *((width,) if wide else ()), hp, hs.size, int(bool(with_ar)), vp, vs.size, float(eps), int(noise_seed), int(row_base), _ptr(out))
    return out


def evaluate(test, prior, h, van_reg, train=None, eps=EPSILON, with_ar=True, noise_seed=0, row_base=0, ws=None):
    """One launch of ``bear_eval_f64``: the 7 partial sums of ``_evaluation_step`` (bear_net.py:323-371).
    Returns a device float64 vector {ll_ear[H], ll_arm, ll_van[V], cor_ear[H], cor_arm, cor_van[V], total_len}."""
    return _evaluate(False, test, prior, h, van_reg, train, eps, with_ar, noise_seed, row_base, ws)


def evaluate_wide(test, prior, h, van_reg, train=None, eps=EPSILON, with_ar=True, noise_seed=0, row_base=0, ws=None):
    """``bear_eval_wide_f64``: ``evaluate`` for rows of width W = ``test.shape[-1]`` (21: the protein alphabet); the same output
    vector, the tie-breaking noise keyed by ``row * W + letter``."""
    return _evaluate(True, test, prior, h, van_reg, train, eps, with_ar, noise_seed, row_base, ws)


class EvalPlan(_Handle):
    """Sorted plan of a resident TEST column (``bear_eval_plan_create``): per tile the cells and row totals with a non-zero
    count, sorted by count, and the rows whose largest counts in the conditioning column ``train`` tie.  Keeps the count
    tensors alive; built asynchronously on the current stream (an evaluation enqueued on ANOTHER stream is not ordered behind the
    build: order the two yourself).  An evaluation launches with the workspace of the stream current at the call (``_step_ws``),
    not with ``self.ws``; destroying the plan frees device memory, which waits for the device."""
    _destroy = "bear_eval_plan_destroy"

    def __init__(self, test, train=None, ws=None):
        test = _check_rows(test, torch.int32, "test")
        if train is not None:
            train = _check_rows(train, torch.int32, "train")
            if train.shape[0] != test.shape[0]:
                raise ValueError("test and train must have the same number of rows")
        self.test, self.train = test, train
        self.ws = ws or default_workspace(test.device)
        with torch.cuda.device(test.device):
            self._create("bear_eval_plan_create", self.ws.handle, _ptr(test), _ptr(train), test.shape[0], after=(_stream(),))

    @property
    def nbytes(self):
        return int(_lib.lib().bear_eval_plan_bytes(self._h))


def evaluate_planned(plan, prior, h, van_reg, eps=EPSILON, with_ar=True, noise_seed=0, row_base=0, row_ids=None):
    """One ``bear_eval_plan_f64`` call: ``evaluate`` on a sorted plan of the test column (same output vector); the conditioning
    column is the one the plan was built with.  ``row_ids`` (int32 storage, uint32 values, [n]): the plan's buffers are a
    compacted batch whose row i is table row ``row_base + row_ids[i]`` (the key of the tie-breaking noise)."""
    test, train = plan.test, plan.train
    n = test.shape[0]
    if row_ids is not None and not (row_ids.is_cuda and row_ids.dtype == torch.int32 and row_ids.is_contiguous()
                                    and row_ids.shape == (n,) and row_ids.data_ptr() % 16 == 0):
        raise ValueError("row_ids must be a contiguous, 16-byte aligned CUDA int32 tensor [n_rows]")
    if prior is not None:
        _check_rows(prior, torch.float64, "prior", n=n, clone=False)
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(van_reg)
    if vs.size and not (1750.0 * float(eps) < 0.5 and (vs >= 0.0).all() and (vs <= 2.0 ** 30).all()):
        raise ValueError("a planned evaluation decides the vanilla models' arg-max on the integer counts: it needs 1750 eps < 0.5 "
                         "and 0 <= van_reg <= 2^30 (kernels.evaluate takes any values)")
    out = torch.empty(2 * (hs.size + vs.size) + 3, dtype=torch.float64, device=test.device)
    _launch(test.device, "bear_eval_plan_f64", _step_ws(plan).handle, plan._h, _ptr(test), _ptr(train), _ptr(prior), n, hp, hs.size,
            int(bool(with_ar)), vp, vs.size, float(eps), int(noise_seed), int(row_base), _ptr(row_ids), _ptr(out))
    return out


def bmm(counts, alpha, ws=None):
    """sum_i lbeta(counts_i + alpha_k) - lbeta(alpha_k) for every alpha_k (dataloader.py:111-118): device [V]."""
    counts = _check_rows(counts, torch.int32, "counts")
    al, ap = _host_f64(alpha)
    ws = ws or default_workspace(counts.device)
    out = torch.empty(al.size, dtype=torch.float64, device=counts.device)
    _launch(counts.device, "bear_bmm_f64", ws.handle, _ptr(counts), counts.shape[0], ap, al.size, _ptr(out))
    return out


TWO_SAMPLE_MAX_MODELS = 16                          # BEAR_TWO_SAMPLE_MAX_MODELS: BEAR and vanilla models of one call
TWO_SAMPLE_TILE = {21: 128, 5: 512}                 # TS_TILE, TS_BLOCKS_PER_CU of kernels_twosample.h: a launch takes
TWO_SAMPLE_BLOCKS_PER_CU = 3                        # min(tiles, blocks per CU * CUs) blocks -- tests size a table beyond that


def _check_bayes_models(h, vans, prior, want_ar):
    """The models of ``two_sample`` and ``k_sample`` as the C ABI takes them -> ``(hs, its pointer), (vans, its pointer)``."""
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(vans)
    if (hs.size or want_ar) and prior is None:
        raise ValueError("the BEAR models (h) and the AR model's likelihood (want_ar) need prior rows")
    if not 1 <= hs.size + vs.size <= TWO_SAMPLE_MAX_MODELS:
        raise ValueError(f"{hs.size} + {vs.size} models: one call takes 1..{TWO_SAMPLE_MAX_MODELS}")
    if not (np.all(hs > 0) and np.all(vs > 0) and np.all(np.isfinite(hs)) and np.all(np.isfinite(vs))):
        raise ValueError("every h and every vanilla pseudo-count must be > 0 and finite")
    return (hs, hp), (vs, vp)


def two_sample(a, b, prior, h, vans, want_ar=False, want_rows=False, ws=None):
    """``bear_two_sample_f64``: the sums of the two-sample and goodness-of-fit Bayes factors over the rows of two count columns
    ``a``, ``b`` [N, W] (uint32 in int32 storage) -> ``(out [H + V, 4] = {M_a, M_b, M_ab, B}, out_ar [2] = {L_a, L_b} or None,
    row_terms [N, H + V] = B_k or None)``, CUDA float64; the H BEAR models (``prior / h``) first, then the V vanilla ones.
    ``prior`` float64 [N, W] or None; ``h``, ``vans``: host values, each > 0 and finite.  One asynchronous call on the current
    stream.  The entry's stream is not its last argument (include/bear_hip.h says why), so the call does not go through
    ``_launch``."""
    a = _check_rows(a, torch.int32, "a", None)
    n, width = a.shape
    b = _check_rows(b, torch.int32, "b", width, n=n)
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", width, n=n)
    if b.device != a.device or (prior is not None and prior.device != a.device):
        raise ValueError("a, b and prior must be on one device")
    (hs, hp), (vs, vp) = _check_bayes_models(h, vans, prior, want_ar)
    ws = ws or default_workspace(a.device)
    out = torch.empty((hs.size + vs.size, 4), dtype=torch.float64, device=a.device)
    out_ar = torch.empty(2, dtype=torch.float64, device=a.device) if want_ar else None
    rows = torch.empty((n, hs.size + vs.size), dtype=torch.float64, device=a.device) if want_rows else None
    with torch.cuda.device(a.device):
        _lib.call("bear_two_sample_f64", ws.handle, _ptr(a), _ptr(b), _ptr(prior), n, width, hp, hs.size, vp, vs.size, _stream(),
                  _ptr(out), _ptr(out_ar), _ptr(rows))
    return out, out_ar, rows


K_SAMPLE_MAX_GROUPS = 16                            # BEAR_K_SAMPLE_MAX_GROUPS: columns of one call
K_SAMPLE_TILES = {21: {2: 128, 4: 64, 8: 48, 16: 24}, 5: {2: 256, 4: 128, 8: 96, 16: 48}}    # KS_TILE(W, GP) of kernels_ksample.h
K_SAMPLE_TILE = {21: 24, 5: 48}                     # ... at sixteen groups, the smallest: a launch takes min(tiles, blocks per CU
K_SAMPLE_BLOCKS_PER_CU = 2                          # * CUs) blocks -- tests size a table beyond that


def k_sample_tile(width, n_groups):
    """The contexts of one tile of ``bear_k_sample_f64`` at ``n_groups`` columns (rounded up to 2, 4, 8 or 16)."""
    return K_SAMPLE_TILES[width][next(g for g in (2, 4, 8, 16) if n_groups <= g)]


def k_sample(counts, cols, prior, h, vans, want_ar=False, want_rows=False, ws=None):
    """``bear_k_sample_f64``: the Bayes factors among the columns ``cols`` (G = 2..16 indices, any subset and order) of the count
    table ``counts`` [C, N, W] (uint32 in int32 storage) in one pass -> ``(out_group [M, G], out_pair [M, P, 2], out_all [M, 2],
    out_ar [G] or None, row_terms [N, M] or None)``, CUDA float64, M = H + V models (BEAR first), the P = G (G - 1) / 2 pairs in the
    order (0, 1), (0, 2), ..., (G - 2, G - 1) of ``cols``; include/bear_hip.h has the formulas.  The table is used in place where
    its rows are contiguous and every chosen column starts on a 16-byte boundary (a ``[C, N, W]`` tensor, or its rows
    ``[:, lo:hi]`` where ``lo * W`` is a multiple of four); any other piece is copied, the chosen columns only.  Outputs and the
    scratch of block partials are allocated here, on the current stream; one asynchronous call (the entry's stream is not its
    last argument: the call does not go through ``_launch``)."""
    if not (torch.is_tensor(counts) and counts.is_cuda and counts.dtype == torch.int32 and counts.dim() == 3):
        raise ValueError("counts must be a CUDA tensor of shape [C, N, W] and dtype torch.int32")
    n_cols, n, width = counts.shape
    if width not in WIDE_WIDTHS:
        raise ValueError(f"counts: rows of width {width}; the kernels take {WIDE_WIDTHS}")
    cols = [int(c) for c in cols]
    if not 2 <= len(cols) <= K_SAMPLE_MAX_GROUPS:
        raise ValueError(f"{len(cols)} columns: one call takes 2..{K_SAMPLE_MAX_GROUPS}")
    if any(not 0 <= c < n_cols for c in cols):
        raise ValueError(f"columns {cols}: the table has {n_cols}")
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", width, n=n)
        if prior.device != counts.device:
            raise ValueError("counts and prior must be on one device")
    (hs, hp), (vs, vp) = _check_bayes_models(h, vans, prior, want_ar)
    dev, G, M = counts.device, len(cols), hs.size + vs.size
    stride = counts.stride(0)
    in_place = n > 0 and counts.stride(2) == 1 and counts.stride(1) == width and stride >= 0 and stride % width == 0 \
        and all((counts.data_ptr() + 4 * c * stride) % 16 == 0 for c in cols)
    if in_place:
        table, col_rows = counts, np.array([c * (stride // width) for c in cols], dtype=np.uint64)
    else:       # the chosen columns, each on a 16-byte boundary: a column of the copy holds a multiple of four rows
        n_pad = max(4, (n + 3) // 4 * 4)
        table = torch.empty((G, n_pad, width), dtype=torch.int32, device=dev)
        for g, c in enumerate(cols):
            table[g, :n] = counts[c]
        col_rows = np.arange(G, dtype=np.uint64) * np.uint64(n_pad)
    ws = ws or default_workspace(dev)
    lib = _lib.lib()
    n_scratch = int(lib.bear_k_sample_scratch(ws.handle, n, width, G))
    scratch = torch.empty(max(n_scratch, 1), dtype=torch.float64, device=dev)
    out_group = torch.empty((M, G), dtype=torch.float64, device=dev)
    out_pair = torch.empty((M, G * (G - 1) // 2, 2), dtype=torch.float64, device=dev)
    out_all = torch.empty((M, 2), dtype=torch.float64, device=dev)
    out_ar = torch.empty(G, dtype=torch.float64, device=dev) if want_ar else None
    rows = torch.empty((n, M), dtype=torch.float64, device=dev) if want_rows else None
    with torch.cuda.device(dev):
        _lib.call("bear_k_sample_f64", ws.handle, _ptr(table), col_rows.ctypes.data_as(ctypes.c_void_p), G, _ptr(prior), n, width,
                  hp, hs.size, vp, vs.size, _stream(), _ptr(scratch), n_scratch, _ptr(out_group), _ptr(out_pair), _ptr(out_all),
                  _ptr(out_ar), _ptr(rows))
    return out_group, out_pair, out_all, out_ar, rows


def synth_counts(seed, row0, n_rows, device, dense=False, want=("train", "test", "ref")):
    """Rows [row0, row0+n_rows) of the synthetic k=13 table, generated on the device."""
    bufs = {k: torch.empty((n_rows, 5), dtype=torch.int32, device=device) for k in want}
    _launch(device, "bear_synth_counts_u32", int(seed), int(row0), int(n_rows), int(bool(dense)), _ptr(bufs.get("train")),
            _ptr(bufs.get("test")), _ptr(bufs.get("ref")))
    return bufs


def synth_prior(seed, row0, n_rows, device):
    prior = torch.empty((n_rows, 5), dtype=torch.float64, device=device)
    _launch(device, "bear_synth_prior_f64", int(seed), int(row0), int(n_rows), _ptr(prior))
    return prior


def synth_kmer_ids(seed, row0, n_rows, lag, device):
    """The k-mers of rows [row0, row0 + n_rows) of the synthetic table as integers in [0, 4^lag) (letter 0 most significant,
    two bits per letter): row index -> a FIXED BIJECTION of [0, 4^lag) -- the contexts of a table are DISTINCT,
    as the contexts of any count table are (summarize.py:429-449 writes one row per k-mer), in a scrambled order, and rows
    [a, b) are the same k-mers however the table is cut into shards.  The bijection: rounds of an odd multiplier + constant
    (mod 4^lag) and a right xor-shift, each invertible on 2 lag bits.  torch ops only: the same numbers on the CPU and the card
    (measurement tooling, like synth_counts; the parity tests draw their own small tables)."""
    lag = int(lag)
    if not 1 <= lag <= 31:
        raise ValueError("synth_kmer_ids: 1 <= lag <= 31")
    bits = 2 * lag
    if row0 < 0 or row0 + n_rows > (1 << bits):
        raise ValueError(f"rows [{row0}, {row0 + n_rows}) of a table of distinct {lag}-mers: only 4^{lag} = {1 << bits} exist")
    mask = (1 << bits) - 1
    x = torch.arange(int(row0), int(row0) + int(n_rows), dtype=torch.int64, device=device)
    s = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & ((1 << 62) - 1)
    for r in range(4):
        mul = ((s >> (7 * r)) | 1) & mask | 1                      # odd: invertible mod 2^bits
        add = (s >> (5 * r + 3)) & mask
        x = (x * mul + add) & mask                                 # (int64 products wrap: the low `bits` bits are exact)
        x = x ^ (x >> max(1, bits // 2 + (r & 1)))
    return x


def synth_kmer_codes(seed, row0, n_rows, lag, device, sort=False):
    """int8 letter codes [n_rows, lag] (0..3 = A, C, G, T: core.encode_kmers) of ``synth_kmer_ids``; ``sort``: in k-mer order
    (the order bear_net.train gives a batch) -- the ids ascending."""
    ids = synth_kmer_ids(seed, row0, n_rows, lag, device)
    if sort:
        ids = torch.sort(ids).values
    shifts = torch.arange(2 * (int(lag) - 1), -1, -2, dtype=torch.int64, device=ids.device)
    return ((ids[:, None] >> shifts[None, :]) & 3).to(torch.int8).contiguous()


def log_gamma(conc, n_samples, seed):
    """One launch of ``bear_log_gamma_f64``: device float64 [n_samples, n] of log Gamma(conc[i], 1) draws."""
    if not (conc.is_cuda and conc.dtype == torch.float64 and conc.dim() == 1 and conc.is_contiguous()):
        raise ValueError("conc must be a contiguous CUDA float64 vector")
    out = torch.empty((int(n_samples), conc.shape[0]), dtype=torch.float64, device=conc.device)
    _launch(conc.device, "bear_log_gamma_f64", _ptr(conc), conc.shape[0], int(n_samples), int(seed) & (2 ** 64 - 1), _ptr(out))
    return out


def _logdir_sample(wide, counts, prior, h, vans, mc_samples, get_map, with_ar, seed, row_base, n_rows, device, width):
    n = None
    if counts is not None:
        counts = _check_rows(counts, torch.int32, "counts", width)
        n, device, width = counts.shape[0], counts.device, counts.shape[1]
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", width)
        if n is not None and prior.shape[0] != n:
            raise ValueError("counts and prior must have the same number of rows")
        n, device, width = prior.shape[0], prior.device, prior.shape[1]
    if n is None:
        if width not in WIDE_WIDTHS:
            raise ValueError(f"width {width}: the wide kernels take {WIDE_WIDTHS}")
        n, device = int(n_rows), torch.device(device or "cuda")
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(vans)
    mc = 1 if get_map else int(mc_samples)
    M = int(bool(with_ar)) + hs.size + vs.size
    out = torch.empty((n, width, M, mc), dtype=torch.float64, device=device)
    _launch(device, "bear_logdir_sample_wide_f64" if wide else "bear_logdir_sample_f64", _ptr(counts), _ptr(prior), n,
            *((int(width),) if wide else ()), hp, hs.size, int(bool(with_ar)), vp, vs.size, mc, int(bool(get_map)),
            int(seed) & (2 ** 64 - 1), int(row_base), _ptr(out))
    return out


def logdir_sample(counts, prior, h, vans, mc_samples, get_map=False, with_ar=False, seed=0, row_base=0, n_rows=None,
                  device=None):
    """One launch of ``bear_logdir_sample_f64``: normalised log transition probabilities
    [n_rows, 5, n_models, mc_samples] (get_var_probs.get_pdf, output='numpy').  counts None = all-zero rows."""
    return _logdir_sample(False, counts, prior, h, vans, mc_samples, get_map, with_ar, seed, row_base, n_rows, device, 5)


def logdir_sample_wide(counts, prior, h, vans, mc_samples, get_map=False, with_ar=False, seed=0, row_base=0, n_rows=None,
                       device=None, width=None):
    """``bear_logdir_sample_wide_f64``: ``logdir_sample`` for rows of width W in ``WIDE_WIDTHS`` (21: the protein alphabet) ->
    [n_rows, W, n_models, mc_samples]; the draw of a cell is keyed by ``(row_base + row) * W + letter``.  W is the width of the
    rows, or ``width`` when both ``counts`` and ``prior`` are None (unseen k-mers, vanilla models only)."""
    return _logdir_sample(True, counts, prior, h, vans, mc_samples, get_map, with_ar, seed, row_base, n_rows, device, width)


# ---- scoring under a sampled table (include/bear_hip.h, "Variant and sequence scoring"; kernels_score.h) ----------------------
# torch has no general uint64 / uint32 arithmetic: keys and offsets travel in int64 storage (a key has at most 63 bits, so the
# signed order is the key order; "no key" reads -1), table rows in int32 storage ("absent" reads -1).
SCORE_BITS = {5: 3, 21: 5}           # key bits per letter at a row width
SCORE_MAX_LAG = {5: 21, 21: 12}      # ... and the longest context one 64-bit key holds
SCORE_SKIP = 0xFF                    # the letter of a position without a transition
SCORE_CHUNK = 2048                   # BEAR_SCORE_CHUNK: transitions of a long segment summed by one wave


def score_ranks(alphabet_name):
    """The rank table of an alphabet of ``core.alphabets_en``: uint8 [W + 1], ``rank[c]`` = position of the character of symbol
    code ``c`` (letters 0 .. W - 2, stop W - 1, start W) among the letters and ``[`` sorted as bytes; 0xFF for the stop, which
    is no letter of a context.  A key packs these ranks, first letter most significant, so keys sort as the k-mer strings do."""
    from . import core
    letters = [str(ch) for ch in core.alphabets_en[alphabet_name][:-1]]
    order = sorted(letters + ["["])
    W = len(letters) + 1
    if W not in WIDE_WIDTHS:
        raise ValueError(f"alphabet {alphabet_name!r}: rows of {W}; the kernels take {WIDE_WIDTHS}")
    rank = np.full(W + 1, 0xFF, dtype=np.uint8)
    for c, ch in enumerate(letters):
        rank[c] = order.index(ch)
    rank[W] = order.index("[")
    return rank


def _check_vec(t, dtype, name, n=None, device=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()
            and (n is None or t.numel() == n) and (device is None or t.device == device)):
        raise ValueError(f"{name} must be a contiguous CUDA {dtype} vector" + ("" if n is None else f" of {n} elements")
                         + ("" if device is None else f" on {device}"))
    return t


def _check_seg(seg, device):
    _check_vec(seg, torch.int64, "seg", device=device)
    if seg.numel() < 1:
        raise ValueError("seg holds n_seg + 1 offsets: at least one")
    return seg.numel() - 1


def score_transitions(text, seg, lag, rank):
    """One launch of ``bear_score_transitions_u64``.  ``text``: CUDA uint8 [n_sym] symbol codes (letters 0 .. W - 2, stop W - 1,
    start W, all written out); ``seg``: CUDA int64 [n_seg + 1] ascending offsets from 0 to n_sym; ``rank``: ``score_ranks`` of the
    alphabet (its length gives W).  Returns ``(keys int64 [n_sym], letters uint8 [n_sym])``: per symbol the key of the ``lag``
    symbols in front of it and its letter index, or -1 / ``SCORE_SKIP`` where it stands less than ``lag`` symbols into its segment."""
    _check_vec(text, torch.uint8, "text")
    n_seg = _check_seg(seg, text.device)
    rank = np.ascontiguousarray(rank, dtype=np.uint8)
    W = rank.size - 1
    if W not in WIDE_WIDTHS:
        raise ValueError(f"rank: {rank.size} entries; a rank table holds W + 1 for W in {WIDE_WIDTHS}")
    if not 1 <= int(lag) <= SCORE_MAX_LAG[W]:
        raise ValueError(f"lag {lag}: a key of {SCORE_BITS[W]} bits per letter holds contexts of 1..{SCORE_MAX_LAG[W]} letters")
    keys = torch.empty(text.numel(), dtype=torch.int64, device=text.device)
    letters = torch.empty(text.numel(), dtype=torch.uint8, device=text.device)
    _launch(text.device, "bear_score_transitions_u64", _ptr(text), _ptr(seg), text.numel(), n_seg, int(lag), W,
            rank.ctypes.data_as(ctypes.c_void_p), _ptr(keys), _ptr(letters))
    return keys, letters


def kmer_find(table, query):
    """One launch of ``bear_kmer_find_u64``: int32 [n_query], the index of every ``query`` key in ``table`` (CUDA int64, ascending
    and distinct, non-negative), -1 where it is absent.  Sorted queries are the fast case; any order is correct."""
    _check_vec(table, torch.int64, "table")
    _check_vec(query, torch.int64, "query", device=table.device)
    if table.numel() >= 2 ** 32 - 1:
        raise ValueError("table: a row index is 32 bits wide")
    rows = torch.empty(query.numel(), dtype=torch.int32, device=table.device)
    _launch(table.device, "bear_kmer_find_u64", _ptr(table), table.numel(), _ptr(query), query.numel(), _ptr(rows))
    return rows


def _check_ref_model(tau, net_weight, eps):
    """The two scalars of a bear_ref model and its epsilon as the C ABI takes them: finite host floats, tau and net_weight > 0."""
    tau, net_weight, eps = float(tau), float(net_weight), float(eps)
    if not (np.isfinite(tau) and tau > 0 and np.isfinite(net_weight) and net_weight > 0):
        raise ValueError("tau and net_weight must be finite and > 0")
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError("eps must be finite and >= 0")
    return tau, net_weight, eps


def _check_ref_table(ref_table, ref_counts, W, device):
    """The reference column as a look-up: ``ref_table`` int64 [N] ascending distinct keys on ``device``, ``ref_counts`` int32 [N, W]
    their count rows in that order (None with an empty table) -> the checked ``ref_counts`` (``_check_rows`` may have copied it)."""
    _check_vec(ref_table, torch.int64, "ref_table", device=device)
    if ref_table.numel() >= 2 ** 32 - 1:
        raise ValueError("ref_table: a row index is 32 bits wide")
    if not ref_table.numel():
        return None
    ref_counts = _check_rows(ref_counts, torch.int32, "ref_counts", W, n=ref_table.numel())
    if ref_counts.device != device:
        raise ValueError(f"ref_counts must be on {device}")
    return ref_counts


def ref_prior_rows(ref_table, ref_counts, query, net_rows, tau, net_weight, eps=EPSILON, width=None):
    """One launch of ``bear_ref_prior_rows_f64``: float64 [n_query, W], the AR function's row of every ``query`` key (CUDA int64, any
    order) under a bear_ref model -- ``(net_weight g + jukes_cantor(ref row, tau)) / (net_weight + 1) + eps`` in the kernel's fixed
    arithmetic (include/bear_hip.h).  ``ref_table`` / ``ref_counts``: the reference column's ascending distinct keys and their int32
    [N, W] count rows in key order (``DeviceCounter.keys`` / ``.counts_by_key``; None with an empty table, then ``width`` says W); an
    absent key has a row of zeros.  ``net_rows``: the net function's rows ``g`` float64 [n_query, W], or None for the stop net
    function.  ``tau``, ``net_weight``: host floats, the model's ``exp(tau_signed)`` and ``exp(net_weight_signed)``."""
    _check_vec(query, torch.int64, "query")
    device = query.device
    W = ref_counts.shape[1] if isinstance(ref_counts, torch.Tensor) and ref_counts.dim() == 2 else width
    if W not in WIDE_WIDTHS:
        raise ValueError(f"rows of width {W}; the kernels take {WIDE_WIDTHS}")
    ref_counts = _check_ref_table(ref_table, ref_counts, W, device)
    tau, net_weight, eps = _check_ref_model(tau, net_weight, eps)
    if net_rows is not None:
        net_rows = _check_rows(net_rows, torch.float64, "net_rows", W, n=query.numel())
        if net_rows.device != device:
            raise ValueError(f"net_rows must be on {device}")
    prior = torch.empty((query.numel(), W), dtype=torch.float64, device=device)
    _launch(device, "bear_ref_prior_rows_f64", _ptr(ref_table), _ptr(ref_counts), ref_table.numel(), W, _ptr(query), query.numel(),
            _ptr(net_rows), tau, net_weight, eps, _ptr(prior))
    return prior


def score_sum(lp, rows, letters, seg):
    """``bear_score_sum_f64``: ``scores[i] = sum_t lp[rows[t], letters[t]]`` over the transitions of segment ``i`` in text order ->
    CUDA float64 [n_seg, M, S].  ``lp``: the sampler's table [K, W, M, S] as ``logdir_sample[_wide]`` returns it; ``rows`` int32
    [n_t] and ``letters`` uint8 [n_t] per position of the text (``SCORE_SKIP``, a negative row: nothing is added); ``seg`` int64
    [n_seg + 1] ascending from 0 to n_t.  Segments beyond ``SCORE_CHUNK`` transitions are summed in chunks, in a fixed order."""
    if not (isinstance(lp, torch.Tensor) and lp.is_cuda and lp.dtype == torch.float64 and lp.dim() == 4 and lp.is_contiguous()
            and lp.shape[1] in WIDE_WIDTHS):
        raise ValueError(f"lp must be a contiguous CUDA float64 tensor [K, W, M, S] with W in {WIDE_WIDTHS}")
    _check_vec(rows, torch.int32, "rows", device=lp.device)
    _check_vec(letters, torch.uint8, "letters", rows.numel(), device=lp.device)
    n_seg = _check_seg(seg, lp.device)
    K, W, M, S = lp.shape
    scores = torch.empty((n_seg, M, S), dtype=torch.float64, device=lp.device)
    _launch(lp.device, "bear_score_sum_f64", _ptr(lp), K, W, M * S, _ptr(rows), _ptr(letters), rows.numel(), _ptr(seg), n_seg,
            _ptr(scores))
    return scores


MARG_CHUNK = 2048                    # BEAR_MARG_CHUNK: positions of a long segment that one wave sums
MARG_MAX_MODELS = 16                 # BEAR_MARG_MAX_MODELS: BEAR and vanilla models of one call


def score_marg(rows, letters, seg, train, prior, h, vans):
    """``bear_score_marg_f64``: the exact Dirichlet-multinomial marginal of every segment -> CUDA float64 [n_seg, H + V], the H BEAR
    models (``prior / h + train``) first, then the V vanilla ones (``van + train``).  ``rows`` int32 [n_t] and ``letters`` uint8 [n_t]
    per position of the text, in TEXT order (``SCORE_SKIP``, a negative row: no transition there); ``seg`` int64 [n_seg + 1]
    ascending from 0 to n_t; ``train`` int32 [K, W] (uint32 in int32 storage) and ``prior`` float64 [K, W] or None: the rows of
    the k-mers the text's rows number; ``h``, ``vans``: host values, each > 0.

    The kernel wants every segment's positions sorted by (row, letter): one ``torch.sort`` of the int64 composite
    ``(segment * (K + 1) + row + 1) * 256 + letter`` (0 and ``SCORE_SKIP`` where there is no transition) does that here, and rows
    and letters are read back out of the sorted values.  ``ValueError`` if the composite would not fit 63 bits."""
    train, prior, n_seg, (hs, hp), (vs, vp) = _check_marg(rows, letters, seg, train, prior, h, vans)
    K, W = train.shape
    device = train.device
    n_t = rows.numel()
    with torch.cuda.device(device):
        rows, letters = _marg_sorted_text(rows, letters, seg, n_seg, K, W)
    scores = torch.empty((n_seg, hs.size + vs.size), dtype=torch.float64, device=device)
    _launch(device, "bear_score_marg_f64", _ptr(rows), _ptr(letters), n_t, _ptr(seg), n_seg, W, _ptr(train), _ptr(prior), K,
            hp, hs.size, vp, vs.size, _ptr(scores))
    return scores


def _check_marg(rows, letters, seg, train, prior, h, vans):
    """What ``score_marg`` and ``score_moments`` check alike -> ``(train, prior, n_seg, (hs, its pointer), (vans, its pointer))``."""
    train = _check_rows(train, torch.int32, "train", None)
    return (train,) + _check_marg_text(rows, letters, seg, train.shape[0], train.shape[1], train.device, prior, h, vans)


def _check_marg_text(rows, letters, seg, K, W, device, prior, h, vans):
    """... and ``score_groups``: everything but the table [K, ..., W] on ``device`` itself -> ``_check_marg``'s result without it."""
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", W, n=K)
    _check_vec(rows, torch.int32, "rows", device=device)
    _check_vec(letters, torch.uint8, "letters", rows.numel(), device=device)
    n_seg = _check_seg(seg, device)
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(vans)
    if hs.size and prior is None:
        raise ValueError("the BEAR models (h) need prior rows")
    if not 1 <= hs.size + vs.size <= MARG_MAX_MODELS:
        raise ValueError(f"{hs.size} + {vs.size} models: one call takes 1..{MARG_MAX_MODELS}")
    if not (np.all(hs > 0) and np.all(vs > 0)):
        raise ValueError("every h and every vanilla pseudo-count must be > 0")
    if max(n_seg, 1) * (K + 1) * 256 >= 2 ** 63:
        raise ValueError(f"{n_seg} segments x {K} k-mers: the sort key (segment, row, letter) does not fit 63 bits")
    return prior, n_seg, (hs, hp), (vs, vp)


def _marg_sort_key(rows, letters, seg, n_seg, K, W):
    """The int64 composite ``(segment * (K + 1) + row + 1) * 256 + letter`` of every position, in text order."""
    n_t = rows.numel()
    live = (rows >= 0) & (rows < K) & (letters < W)
    segment = torch.searchsorted(seg[1:], torch.arange(n_t, dtype=torch.int64, device=rows.device), right=True).clamp_(max=max(n_seg - 1, 0))
    return (segment * (K + 1) + torch.where(live, rows.to(torch.int64) + 1, 0)) * 256 + torch.where(live, letters.to(torch.int64), SCORE_SKIP)


def _marg_sorted_text(rows, letters, seg, n_seg, K, W, want_order=False):
    """One ``torch.sort`` of ``_marg_sort_key``, rows and letters read back out of the sorted values -> ``(rows int32, letters uint8)``
    sorted inside every segment by (row, letter), and with ``want_order`` the sort's permutation.  Under the caller's device context."""
    key, order = torch.sort(_marg_sort_key(rows, letters, seg, n_seg, K, W))
    if not want_order:
        order = None                     # freed in front of the read-back's temporaries
    letters = (key & 0xFF).to(torch.uint8)
    rows = (torch.div(key, 256, rounding_mode="floor") % (K + 1) - 1).to(torch.int32)
    return (rows, letters) if order is None else (rows, letters, order)


GROUPS_MAX = 256                     # BEAR_GROUPS_MAX: groups (columns) of the table of one bear_score_groups_f64 call


def score_groups(rows, letters, seg, train, prior, h, vans, own=None):
    """``bear_score_groups_f64``: ``score_marg`` under every group of a count table at once -> ``(scores [n_seg, G, H + V] CUDA float64,
    short_of [n_seg] CUDA uint8)``.  The arguments of ``score_marg``, except ``train``: int32 [K, G, W] (uint32 in int32 storage), the
    G count rows of a k-mer adjacent; and ``own``: int32 [n_seg] on the device or None -- the group whose counts contain the segment
    itself (negative, or >= G: none), which is scored with the segment's own counts taken out of it (leave-one-out).
    ``short_of[s]`` = 1: segment ``s`` has a transition more often than its own group holds it, its own-group scores are NaN.

    The composite-key sort of ``score_marg``; one asynchronous call on the current stream.  The entry's stream is not its last
    argument (include/bear_hip.h says why), so the call does not go through ``_launch``."""
    if not (isinstance(train, torch.Tensor) and train.is_cuda and train.dtype == torch.int32 and train.dim() == 3
            and train.is_contiguous() and train.shape[2] in WIDE_WIDTHS):
        raise ValueError(f"train must be a contiguous CUDA int32 tensor [K, G, W] with W in {WIDE_WIDTHS}")
    K, G, W = train.shape
    if not 1 <= G <= GROUPS_MAX:
        raise ValueError(f"{G} groups: one call takes 1..{GROUPS_MAX}")
    if train.data_ptr() % 16:
        train = train.clone()
    device = train.device
    prior, n_seg, (hs, hp), (vs, vp) = _check_marg_text(rows, letters, seg, K, W, device, prior, h, vans)
    if own is not None:
        _check_vec(own, torch.int32, "own", n_seg, device=device)
    n_t = rows.numel()
    if max(n_seg, 1) * G * (hs.size + vs.size) * 8 >= 2 ** 63 or max(n_t, 1) * G * (hs.size + vs.size) * 8 >= 2 ** 63:
        raise ValueError(f"{n_seg} segments, {n_t} positions x {G} groups x {hs.size + vs.size} models: too many terms for one call")
    with torch.cuda.device(device):
        rows, letters = _marg_sorted_text(rows, letters, seg, n_seg, K, W)
        scores = torch.empty((n_seg, G, hs.size + vs.size), dtype=torch.float64, device=device)
        short_of = torch.empty(n_seg, dtype=torch.uint8, device=device)
        _lib.call("bear_score_groups_f64", _ptr(rows), _ptr(letters), n_t, _ptr(seg), n_seg, W, _ptr(train), G, _ptr(prior), K, _ptr(own),
                  hp, hs.size, vp, vs.size, _stream(), _ptr(scores), _ptr(short_of))
    return scores, short_of


HMM_MAX_STATES = 16                  # BEAR_HMM_MAX_STATES: states of the chain of one bear_hmm_groups_f64 call
HMM_CHUNK = 512                      # BEAR_HMM_CHUNK: steps of a segment that one lane group runs front to back and back


def emit_groups(rows, letters, train, prior, h, vans):
    """``bear_score_emit_groups_f64``: the posterior-predictive log-probability of every position's letter under every group and
    model -> CUDA float64 [H + V, n_t, G], the H BEAR models first; plane ``m`` is the ``emit`` of ``hmm_groups``.  ``rows`` int32
    [n_t] and ``letters`` uint8 [n_t] per position in TEXT order (nothing is sorted); ``train`` int32 [K, G, W], ``prior`` float64
    [K, W] or None, ``h`` and ``vans`` as ``score_groups`` takes them.  A position without a transition (``SCORE_SKIP``, a negative
    row, a row >= K) holds exactly 0.0.  One asynchronous call on the current stream (the entry's stream is not its last argument)."""
    if not (isinstance(train, torch.Tensor) and train.is_cuda and train.dtype == torch.int32 and train.dim() == 3
            and train.is_contiguous() and train.shape[2] in WIDE_WIDTHS):
        raise ValueError(f"train must be a contiguous CUDA int32 tensor [K, G, W] with W in {WIDE_WIDTHS}")
    K, G, W = train.shape
    if not 1 <= G <= GROUPS_MAX:
        raise ValueError(f"{G} groups: one call takes 1..{GROUPS_MAX}")
    if train.data_ptr() % 16:
        train = train.clone()
    device = train.device
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", W, n=K)
    _check_vec(rows, torch.int32, "rows", device=device)
    _check_vec(letters, torch.uint8, "letters", rows.numel(), device=device)
    (hs, hp), (vs, vp) = _host_f64(h), _host_f64(vans)
    if hs.size and prior is None:
        raise ValueError("the BEAR models (h) need prior rows")
    if not 1 <= hs.size + vs.size <= MARG_MAX_MODELS:
        raise ValueError(f"{hs.size} + {vs.size} models: one call takes 1..{MARG_MAX_MODELS}")
    if not (np.all(hs > 0) and np.all(vs > 0)):
        raise ValueError("every h and every vanilla pseudo-count must be > 0")
    n_t, M = rows.numel(), hs.size + vs.size
    if max(n_t, 1) * G * M * 8 >= 2 ** 63:
        raise ValueError(f"{n_t} positions x {G} groups x {M} models: too many values for one call")
    with torch.cuda.device(device):
        emit = torch.empty((M, n_t, G), dtype=torch.float64, device=device)
        _lib.call("bear_score_emit_groups_f64", _ptr(rows), _ptr(letters), n_t, W, _ptr(train), G, _ptr(prior), K, hp, hs.size, vp, vs.size,
                  _stream(), _ptr(emit))
    return emit


def check_chain(log_trans, log_start, n_states):
    """The chain of ``hmm_groups`` as the C ABI takes it -> ``(log_trans float64 [S, S], log_start float64 [S])``, C-contiguous host
    arrays.  -inf is allowed and rows need not be normalised; ``ValueError`` for a wrong shape, a NaN or +inf, a row or a start
    without a finite entry, or S outside 1..``HMM_MAX_STATES``.  Needs no device."""
    S = int(n_states)
    if not 1 <= S <= HMM_MAX_STATES:
        raise ValueError(f"{S} states: a chain has 1..{HMM_MAX_STATES}")
    log_trans = np.ascontiguousarray(np.asarray(log_trans, dtype=np.float64))
    log_start = np.ascontiguousarray(np.asarray(log_start, dtype=np.float64))
    if log_trans.shape != (S, S) or log_start.shape != (S,):
        raise ValueError(f"log_trans must be [{S}, {S}] (from-state by row) and log_start [{S}]")
    for name, a in (("log_trans", log_trans), ("log_start", log_start[None, :])):
        if np.isnan(a).any() or np.isposinf(a).any():
            raise ValueError(f"{name}: log probabilities (-inf rules a step out), no NaN and no +inf")
        if not np.isfinite(a).any(axis=1).all():
            raise ValueError(f"{name}: every row needs a finite entry")
    return log_trans, log_start


def hmm_groups(emit, seg, log_trans, log_start, want_post=True):
    """``bear_hmm_groups_f64``: a hidden-Markov chain over the S states along every segment -> ``(log_evidence [n_seg] float64,
    log_best [n_seg] float64, path [n_t] uint8, log_post [n_t, S] float64 or None)``, CUDA tensors.  ``emit``: contiguous CUDA
    float64 [n_t, S], the log-probability of step ``t`` under state ``g``; ``seg`` int64 [n_seg + 1] ascending from 0 to n_t -- it
    MUST cover the text: the offsets live on the device, so they are not checked here, and ``path`` / ``log_post`` of a step that no
    segment covers are returned as allocated, unwritten;
    ``log_trans`` [S, S] from-state by row and ``log_start`` [S]: host values (``check_chain``).  ``path[t]``: the lowest state of
    the largest max-marginal, 255 where every path is -inf; ``log_post``: every step's posterior over the states
    (``want_post=False``: not formed).  Segments beyond ``HMM_CHUNK`` steps run in chunks (include/bear_hip.h, the chunk rule).
    One asynchronous call on the current stream."""
    if not (isinstance(emit, torch.Tensor) and emit.is_cuda and emit.dtype == torch.float64 and emit.dim() == 2 and emit.is_contiguous()):
        raise ValueError("emit must be a contiguous CUDA float64 tensor [n_t, S]")
    n_t, S = emit.shape
    log_trans, log_start = check_chain(log_trans, log_start, S)
    device = emit.device
    n_seg = _check_seg(seg, device)
    if emit.data_ptr() % 8:
        emit = emit.clone()
    with torch.cuda.device(device):
        log_evidence = torch.empty(n_seg, dtype=torch.float64, device=device)
        log_best = torch.empty(n_seg, dtype=torch.float64, device=device)
        path = torch.empty(n_t, dtype=torch.uint8, device=device)
        log_post = torch.empty((n_t, S), dtype=torch.float64, device=device) if want_post else None
        _lib.call("bear_hmm_groups_f64", _ptr(emit), n_t, _ptr(seg), n_seg, S, log_trans.ctypes.data_as(ctypes.c_void_p),
                  log_start.ctypes.data_as(ctypes.c_void_p), _stream(), _ptr(log_evidence), _ptr(log_best), _ptr(path), _ptr(log_post))
    return log_evidence, log_best, path, log_post


def score_moments(rows, letters, seg, train, prior, h, vans, weights=None):
    """``bear_score_moments_f64``: the exact posterior mean and variance of every segment's score -> CUDA float64 [n_seg, H + V, 2]
    (``[..., 0]`` the mean, ``[..., 1]`` the variance as summed, not clamped), the models in ``score_marg``'s order.  With
    ``p ~ Dirichlet(a)`` the row of a k-mer under a model (``a`` as ``score_marg`` forms it), a segment's score is the sum over its
    transitions of ``w log p[letter]``; different k-mers are independent.  The arguments of ``score_marg``, and ``weights``: int8
    [n_t] of +1 / -1 in text order (a mutant window's transitions count for the score, the wild type's against it), None for all +1.

    The sort of ``score_marg`` carries the weights along; their prefix sum over the sorted text (one ``torch.cumsum``) gives the
    kernel the signed count of any run in two loads."""
    train, prior, n_seg, (hs, hp), (vs, vp) = _check_marg(rows, letters, seg, train, prior, h, vans)
    K, W = train.shape
    device = train.device
    n_t = rows.numel()
    if weights is not None:
        _check_vec(weights, torch.int8, "weights", n_t, device=device)
    prefix = None
    with torch.cuda.device(device):
        rows, letters, order = _marg_sorted_text(rows, letters, seg, n_seg, K, W, want_order=True)
        if weights is not None:
            if n_t and not bool((weights.abs() == 1).all()):
                raise ValueError("weights: every entry is +1 or -1")
            prefix = torch.zeros(n_t + 1, dtype=torch.int64, device=device)
            torch.cumsum(weights[order], 0, dtype=torch.int64, out=prefix[1:])
    moments = torch.empty((n_seg, hs.size + vs.size, 2), dtype=torch.float64, device=device)
    _launch(device, "bear_score_moments_f64", _ptr(rows), _ptr(letters), _ptr(prefix), n_t, _ptr(seg), n_seg, W, _ptr(train),
            _ptr(prior), K, hp, hs.size, vp, vs.size, _ptr(moments))
    return moments


# ---- sequence generation over a key table (include/bear_hip.h, "Sequence generation"; kernels_generate.h) ----------------------
GEN_BMM, GEN_BEAR, GEN_AR = 0, 1, 2  # BEAR_GEN_*: where a letter's concentration comes from
GEN_ID_GUMBEL = 3000                 # the model id that keys the Gumbel draws (the table values are model 0)
GEN_NET_STOP, GEN_NET_ROWS, GEN_NET_MAT = 0, 1, 2      # BEAR_GEN_NET_*: where a bear_ref model's net rows come from


def _generate_launch(entry, table, counts, rank, lag, keys, sample, left, letters, step0, n_steps, seed, van, prior, h, get_map, codes,
                     mat=None, state=None, ref=None):
    """What ``generate_steps`` and ``generate_whole`` check alike, and the launch of ``entry`` with its complete argument list.
    ``state`` = (length, stopped) says ``bear_generate_whole_f64``: it takes ``mat`` behind ``prior`` and the state behind ``left``.
    ``ref`` = (ref_table, ref_counts, tau, net_weight, eps) says ``bear_generate_whole_ref_f64``: ``prior`` / ``mat`` are then the net
    function's rows (neither: the stop net function), and the reference column and the model's scalars go behind ``codes``.
    The checked ``counts`` and ``prior`` (``_check_rows`` may have copied them) live in this frame across the launch."""
    _check_vec(table, torch.int64, "table")
    device = table.device
    rank = np.ascontiguousarray(rank, dtype=np.uint8)
    W = rank.size - 1
    if W not in WIDE_WIDTHS:
        raise ValueError(f"rank: {rank.size} entries; a rank table holds W + 1 for W in {WIDE_WIDTHS}")
    if not 1 <= int(lag) <= SCORE_MAX_LAG[W]:
        raise ValueError(f"lag {lag}: a key of {SCORE_BITS[W]} bits per letter holds contexts of 1..{SCORE_MAX_LAG[W]} letters")
    if table.numel():
        counts = _check_rows(counts, torch.int32, "counts", W, n=table.numel())
    else:
        counts = None
    n = keys.numel() if isinstance(keys, torch.Tensor) else -1
    _check_vec(keys, torch.int64, "keys", device=device)
    _check_vec(sample, torch.int64, "sample", n, device=device)
    _check_vec(left, torch.int32, "left", n, device=device)
    step0, n_steps = int(step0), int(n_steps)
    if step0 < 0 or n_steps < 0:
        raise ValueError("step0 and n_steps count steps: not negative")
    if not (isinstance(letters, torch.Tensor) and letters.device == device and letters.dtype == torch.uint8 and letters.dim() == 2
            and letters.is_contiguous() and letters.shape[0] == n):
        raise ValueError(f"letters must be a contiguous CUDA uint8 tensor [{n}, L] on {device}")
    if letters.shape[1] < step0 + n_steps:
        raise ValueError(f"letters: rows of {letters.shape[1]}, steps {step0} .. {step0 + n_steps} do not fit")
    if prior is not None:
        prior = _check_rows(prior, torch.float64, "prior", W, n=n)
        if prior.device != device:
            raise ValueError(f"prior must be on {device}")
        if n_steps > 1:
            raise ValueError("prior rows belong to the current end k-mers: one step per launch")
    if ref is not None:
        if van is not None:
            raise ValueError("a reference model mixes an AR function's rows: no BMM (van)")
        ref_counts = _check_ref_table(ref[0], ref[1], W, device)
        ref_scalars = _check_ref_model(*ref[2:])
    if prior is not None or mat is not None or ref is not None:
        if h is None and not get_map:
            raise ValueError("the AR model (rows without h) is a table only at its MAP value: get_map=True")
        mode = GEN_AR if h is None else GEN_BEAR
    elif van is None:
        raise ValueError("a BMM (van=...) or rows of an AR function")
    else:
        mode = GEN_BMM
    if mode == GEN_BEAR and not float(h) > 0 or mode == GEN_BMM and not float(van) > 0:
        raise ValueError("h and van must be > 0")
    if codes is not None and not (isinstance(codes, torch.Tensor) and codes.device == device and codes.dtype == torch.int8
                                  and codes.is_contiguous() and tuple(codes.shape) == (n, int(lag))):
        raise ValueError(f"codes must be a contiguous CUDA int8 tensor [{n}, {int(lag)}] on {device}")
    whole = state is not None
    if whole:
        _check_vec(state[0], torch.int32, "length", n, device=device)
        _check_vec(state[1], torch.uint8, "stopped", n, device=device)
    if mat is not None:
        if W != LINEAR_WIDE_WIDTH:
            raise ValueError(f"mat: the linear AR function runs inside the kernel at rows of {LINEAR_WIDE_WIDTH} only")
        if not (isinstance(mat, torch.Tensor) and mat.device == device and mat.dtype == torch.float64 and mat.is_contiguous()
                and tuple(mat.shape) == (int(lag), W, W)):
            raise ValueError(f"mat must be a contiguous CUDA float64 tensor [{int(lag)}, {W}, {W}] on {device}")
    _launch(device, entry, _ptr(table), _ptr(counts), table.numel(), int(lag), W, rank.ctypes.data_as(ctypes.c_void_p), mode,
            int(bool(get_map)), float(h) if mode == GEN_BEAR else 0.0, float(van) if mode == GEN_BMM else 0.0, _ptr(prior),
            *([_ptr(mat)] if whole else []), int(seed) & (2 ** 64 - 1), _ptr(keys), _ptr(sample), _ptr(left),
            *([_ptr(state[0]), _ptr(state[1])] if whole else []), n, step0, n_steps, _ptr(letters), letters.shape[1], _ptr(codes),
            *([] if ref is None else [_ptr(ref[0]), _ptr(ref_counts), ref[0].numel(), *ref_scalars,
                                      GEN_NET_ROWS if prior is not None else (GEN_NET_MAT if mat is not None else GEN_NET_STOP)]))


def generate_steps(table, counts, rank, lag, keys, sample, left, letters, step0, n_steps, seed, van=None, prior=None, h=None,
                   get_map=False, codes=None):
    """One launch of ``bear_generate_steps_f64``: steps ``step0 .. step0 + n_steps - 1`` of every sequence that has letters left.
    ``table``: CUDA int64 [N] ascending distinct keys, ``counts`` int32 [N, W] their count rows in that order (None with an empty
    table); ``rank``: ``score_ranks`` of the alphabet.  Per sequence, all on the table's device and updated in place: ``keys``
    int64 [n] the end key, ``left`` int32 [n] the letters still to write; ``sample`` int64 [n] the sample index; ``letters`` uint8
    [n, L >= step0 + n_steps] receives the letter codes at columns ``step0 ..``.  The model: ``van`` (a BMM: any ``n_steps``, a whole
    flank in one launch), or ``prior`` float64 [n, W] rows of the current end k-mers (``n_steps`` 1) with ``h`` (BEAR) or without
    (the AR model, ``get_map`` only).  ``codes`` int8 [n, lag], if given, receives the new end k-mers as ``core.encode_kmers`` codes."""
    _generate_launch("bear_generate_steps_f64", table, counts, rank, lag, keys, sample, left, letters, step0, n_steps, seed, van, prior,
                     h, get_map, codes)


def generate_whole(table, counts, rank, lag, keys, sample, left, length, stopped, letters, step0, n_steps, seed, van=None, prior=None,
                   mat=None, h=None, get_map=False, codes=None):
    """One launch of ``bear_generate_whole_f64``: ``generate_steps`` with the stop drawn like a letter.  A sequence that has steps
    ``left`` (int32 [n]: the cut) takes them until the stop wins: then ``stopped`` (uint8 [n]) is set, ``left`` becomes 0, nothing is
    written and the key stays; a letter goes to ``letters`` and adds 1 to ``length`` (int32 [n]).  ``keys``, ``left``, ``length`` and
    ``stopped`` are the whole state, updated in place.  The model: ``van``; ``prior`` rows of the current end k-mers (``n_steps`` 1); or,
    for the protein alphabet, ``mat`` float64 [lag, 21, 21] -- the linear AR function inside the kernel, any ``n_steps`` -- the last
    two with ``h`` (BEAR) or without (the AR model, ``get_map`` only)."""
    if prior is not None and mat is not None:
        raise ValueError("prior rows or mat: one source of the AR function's rows")
    _generate_launch("bear_generate_whole_f64", table, counts, rank, lag, keys, sample, left, letters, step0, n_steps, seed, van, prior,
                     h, get_map, codes, mat=mat, state=(length, stopped))


def generate_whole_ref(table, counts, ref_table, ref_counts, rank, lag, keys, sample, left, length, stopped, letters, step0, n_steps, seed,
                       tau, net_weight, net_rows=None, mat=None, h=None, get_map=False, codes=None, eps=EPSILON):
    """One launch of ``bear_generate_whole_ref_f64``: ``generate_whole`` under a bear_ref model.  The AR function's row of an end
    k-mer is formed inside the step, as ``ref_prior_rows`` forms it, from the k-mer's row in the reference column (``ref_table`` /
    ``ref_counts``, as there) and the net function's row: the one-hot at the stop (neither ``net_rows`` nor ``mat``: any ``n_steps``,
    whole sequences in one launch), ``net_rows`` float64 [n, W] of the current end k-mers (``n_steps`` 1), or, for the protein
    alphabet, the linear function of ``mat`` [lag, 21, 21] inside the kernel (any ``n_steps``).  With ``h`` a BEAR model, without the
    AR model (``get_map`` only)."""
    if net_rows is not None and mat is not None:
        raise ValueError("net_rows or mat: one source of the net function's rows")
    _generate_launch("bear_generate_whole_ref_f64", table, counts, rank, lag, keys, sample, left, letters, step0, n_steps, seed, None,
                     net_rows, h, get_map, codes, mat=mat, state=(length, stopped), ref=(ref_table, ref_counts, tau, net_weight, eps))


def shuffle_rows(src, seed):
    """One launch of ``bear_shuffle_rows``: a new tensor with ``dst[i] = src[perm_seed(i)]`` along dim 0."""
    if not (src.is_cuda and src.is_contiguous() and src.dim() >= 1):
        raise ValueError("src must be a contiguous CUDA tensor")
    dst = torch.empty_like(src)
    n = src.shape[0]
    row_bytes = src.element_size() * (src.numel() // n) if n else 0
    _launch(src.device, "bear_shuffle_rows", _ptr(src), _ptr(dst), n, row_bytes, int(seed) & (2 ** 64 - 1))
    return dst


def shuffle_rows_range(src, first, n_out, seed, n_rows=None, row_shape=None, dtype=None, out=None):
    """One launch of ``bear_shuffle_rows_range`` on the current stream: ``dst[j] = src[perm_seed(first + j)]`` for ``j < n_out``
    along dim 0 -- rows ``[first, first + n_out)`` of ``shuffle_rows(src, seed)``.  ``src``: a contiguous CUDA tensor; ``n_rows``
    / ``row_shape`` / ``dtype`` (of the source's element size) describe its bytes as rows and default to the tensor's own.
    ``out``: the destination, a contiguous CUDA tensor ``[n_out, *row_shape]``; a new one otherwise."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dim() >= 1):
        raise ValueError("src must be a contiguous CUDA tensor")
    device, item = src.device, src.element_size()
    dtype = src.dtype if dtype is None else dtype
    n_rows = src.shape[0] if n_rows is None else int(n_rows)
    row_shape = tuple(src.shape[1:]) if row_shape is None else tuple(row_shape)
    first, n_out = int(first), int(n_out)
    row_elems = int(np.prod(row_shape, dtype=np.int64))
    if torch.empty(0, dtype=dtype).element_size() != item or n_rows * row_elems != src.numel():
        raise ValueError("n_rows, row_shape and dtype must describe the source's own bytes")
    if not (0 <= first and 0 <= n_out and first + n_out <= n_rows):
        raise ValueError(f"rows [{first}, {first + n_out}) of {n_rows}")
    if out is None:
        out = torch.empty((n_out,) + row_shape, dtype=dtype, device=device)
    elif not (isinstance(out, torch.Tensor) and out.device == device and out.is_contiguous() and out.dtype == dtype
              and tuple(out.shape) == (n_out,) + row_shape):
        raise ValueError(f"out must be a contiguous {dtype} tensor {(n_out,) + row_shape} on {device}")
    _launch(device, "bear_shuffle_rows_range", _ptr(src), _ptr(out), n_rows, first, n_out, item * row_elems, int(seed) & (2 ** 64 - 1))
    return out


HOST_GATHER_THREADS = 16


def shuffle_gather_host(array, first, n_out, seed, n_threads=HOST_GATHER_THREADS):
    """``bear_shuffle_gather_host``: rows ``perm_seed(first) .. perm_seed(first + n_out - 1)`` of the C-contiguous NumPy ``array``
    (along axis 0) as a new array, gathered by ``n_threads`` host threads.  Needs no device."""
    if not (isinstance(array, np.ndarray) and array.flags.c_contiguous and array.ndim >= 1):
        raise ValueError("a C-contiguous NumPy array")
    n = array.shape[0]
    first, n_out = int(first), int(n_out)
    out = np.empty((max(n_out, 0),) + array.shape[1:], dtype=array.dtype)
    row_bytes = array.nbytes // n if n else 0
    _lib.call("bear_shuffle_gather_host", ctypes.c_void_p(array.ctypes.data), ctypes.c_void_p(out.ctypes.data), n, first & (2 ** 64 - 1),
              n_out & (2 ** 64 - 1), row_bytes, int(seed) & (2 ** 64 - 1), int(n_threads))
    return out


def kmer_order(kmer_code, lag):
    """``bear_kmer_order_u64``: int32-storage permutation [n] that sorts packed contexts (``pack_kmers``) lexicographically, first
    letter most significant, stable.  Stream-ordered: the sort's scratch (``kmer_order_scratch_bytes``: ~20 B per row) is a torch
    tensor, so it comes out of -- and goes back to -- the caching allocator like every other slab."""
    _check_codes(kmer_code)
    n = kmer_code.shape[0]
    perm = torch.empty(n, dtype=torch.int32, device=kmer_code.device)
    nbytes = ctypes.c_uint64(kmer_order_scratch_bytes(n, lag))
    scratch = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=kmer_code.device)
    _launch(kmer_code.device, "bear_kmer_order_u64", _ptr(kmer_code), n, int(lag), _ptr(perm), _ptr(scratch), ctypes.byref(nbytes))
    return perm


def kmer_order_scratch_bytes(n_rows, lag):
    """Device scratch ``bear_kmer_order_u64`` asks of its caller for a batch of n_rows contexts."""
    nbytes = ctypes.c_uint64(0)
    _lib.call("bear_kmer_order_u64", None, int(n_rows), int(lag), None, None, ctypes.byref(nbytes), _stream())   # (a size query launches nothing)
    return int(nbytes.value)


def gather_rows(src, perm):
    """One launch of ``bear_gather_rows``: a new tensor with ``dst[i] = src[perm[i]]`` along dim 0 (perm: int32 storage)."""
    if not (src.is_cuda and src.is_contiguous() and src.dim() >= 1 and perm.is_cuda and perm.dtype == torch.int32
            and perm.is_contiguous() and perm.shape == (src.shape[0],)):
        raise ValueError("src: contiguous CUDA tensor; perm: contiguous CUDA int32 [n_rows]")
    dst = torch.empty_like(src)
    n = src.shape[0]
    row_bytes = src.element_size() * (src.numel() // n) if n else 1
    _launch(src.device, "bear_gather_rows", _ptr(src), _ptr(perm), _ptr(dst), n, row_bytes)
    return dst


def shuffle_source_row(i, n_rows, seed):
    """Host evaluation of the permutation: the source row of shuffled row i."""
    return int(_lib.lib().bear_shuffle_source_row(int(i), int(n_rows), int(seed) & (2 ** 64 - 1)))


CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, CNN_MAX_LAG = 30, 16, 21   # CNN_NF / CNN_L1 / CNN_MAX_LAG of kernels_cnn.h


CNN_WIDE_MAX_LAG = 16      # CNN_WIDE_MAX_LAG of include/bear_hip.h (the filter image and a tile's staged rows live in LDS)


def cnn_supported(lag, alphabet_size, filter_width, num_filters, kmer_layer1_width):
    """The convolutional AR function has HIP kernels for the 4-letter alphabets (packed contexts) and, as rows, for the protein
    alphabet (int8 codes).  At width 21, forward + backward measured 13x to 100x faster than the torch formulation at every shape
    timed -- lag / filter width 1/1, 4/1, 5/3, 12/8, 16/8 at 1e6 and 1e7 contexts (profiles/prot_cnn_time.jsonl) --
    so every shape the kernels take is covered."""
    if not (num_filters == CNN_NUM_FILTERS and kmer_layer1_width == CNN_LAYER1_WIDTH):
        return False
    if alphabet_size == 20:
        return 1 <= filter_width <= lag <= CNN_WIDE_MAX_LAG
    return alphabet_size == 4 and 1 <= filter_width <= lag <= CNN_MAX_LAG


def _count(name, *args):
    """A size query: the entry ``name`` answers a count, or a negative status."""
    n = getattr(_lib.lib(), name)(*args)
    _lib.check(min(n, 0), name)
    return n


def cnn_param_count(lag, filter_width):
    return _count("bear_cnn_param_count", int(lag), int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH)


def _check_codes(kmer_code):
    if not (kmer_code.is_cuda and kmer_code.dtype == torch.int64 and kmer_code.dim() == 1 and kmer_code.is_contiguous()):
        raise ValueError("kmer_code must be a contiguous CUDA int64 tensor [n_rows] (pack_kmers)")


def cnn_forward(kmer_code, flat_params, lag, filter_width, save=True, ws=None, plan=None):
    """One launch of ``bear_cnn_forward_f64``: (prior [n,5], t1 [n,16] or None).  ``plan``: a plan of the same rows -- the forward
    pass then runs over its prefix levels when they were attached for this tensor (``bear_cnn_forward_plan_f64``; t1 is kept)."""
    _check_codes(kmer_code)
    n = kmer_code.shape[0]
    if not (flat_params.is_cuda and flat_params.dtype == torch.float64 and flat_params.is_contiguous()
            and flat_params.numel() == cnn_param_count(lag, filter_width)):
        raise ValueError("flat_params must be the contiguous CUDA float64 parameter vector of bear_cnn_param_count elements")
    if plan is not None:
        if plan.counts.shape[0] != n:
            raise ValueError("plan: built for another number of rows than kmer_code holds")
        prior = torch.empty((n, 5), dtype=torch.float64, device=kmer_code.device)
        t1 = torch.empty((n, CNN_LAYER1_WIDTH), dtype=torch.float64, device=kmer_code.device)
        _launch(kmer_code.device, "bear_cnn_forward_plan_f64", _step_ws(plan).handle, plan._h, _ptr(kmer_code), n, int(lag), int(filter_width),
                CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, _ptr(flat_params), _ptr(prior), _ptr(t1))
        return prior, t1
    ws = ws or default_workspace(kmer_code.device)
    prior = torch.empty((n, 5), dtype=torch.float64, device=kmer_code.device)
    t1 = torch.empty((n, CNN_LAYER1_WIDTH), dtype=torch.float64, device=kmer_code.device) if save else None
    _launch(kmer_code.device, "bear_cnn_forward_f64", ws.handle, _ptr(kmer_code), n, int(lag), int(filter_width), CNN_NUM_FILTERS,
            CNN_LAYER1_WIDTH, _ptr(flat_params), _ptr(prior), _ptr(t1))
    return prior, t1


def cnn_backward(kmer_code, flat_params, lag, filter_width, t1, prior, grad_prior, ws=None):
    """One launch of ``bear_cnn_backward_f64``: d L / d flat_params."""
    _check_codes(kmer_code)
    n = kmer_code.shape[0]
    for t, w in ((t1, CNN_LAYER1_WIDTH), (prior, 5), (grad_prior, 5)):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n, w)):
            raise ValueError("t1 [n,16], prior [n,5] and grad_prior [n,5] must be contiguous CUDA float64 tensors")
    ws = ws or default_workspace(kmer_code.device)
    grad = torch.empty_like(flat_params)
    _launch(kmer_code.device, "bear_cnn_backward_f64", ws.handle, _ptr(kmer_code), n, int(lag), int(filter_width), CNN_NUM_FILTERS,
            CNN_LAYER1_WIDTH, _ptr(flat_params), _ptr(t1), _ptr(prior), _ptr(grad_prior), _ptr(grad))
    return grad


LINEAR_WIDE_MAX_LAG = 16   # LINEAR_WIDE_MAX_LAG of include/bear_hip.h (mat [lag, 21, 21] lives in LDS)
LINEAR_WIDE_WIDTH = 21     # the protein alphabet: 20 letters + stop


def linear_supported(lag, alphabet_size):
    """The linear AR function has HIP rows for the 4-letter alphabets (packed contexts) and for the protein alphabet (int8 codes)."""
    if alphabet_size == 20:
        return 1 <= lag <= LINEAR_WIDE_MAX_LAG
    return alphabet_size == 4 and 1 <= lag <= LINEAR_MAX_LAG


def _check_mat(mat, lag):
    if not (mat.is_cuda and mat.dtype == torch.float64 and mat.is_contiguous() and tuple(mat.shape) == (lag, 5, 5)):
        raise ValueError("mat must be a contiguous CUDA float64 tensor [lag, 5, 5]")


def linear_forward(kmer_code, mat, lag, ws=None):
    """One launch of ``bear_linear_forward_f64``: the rows softmax(sum_l mat[l, kmer[l], :]) [n, 5] of packed contexts."""
    _check_codes(kmer_code)
    _check_mat(mat, lag)
    n = kmer_code.shape[0]
    ws = ws or default_workspace(kmer_code.device)
    prior = torch.empty((n, 5), dtype=torch.float64, device=kmer_code.device)
    _launch(kmer_code.device, "bear_linear_forward_f64", ws.handle, _ptr(kmer_code), n, int(lag), _ptr(mat), _ptr(prior))
    return prior


def linear_backward(kmer_code, lag, prior, grad_prior, ws=None):
    """One launch of ``bear_linear_backward_f64``: d L / d mat [lag, 5, 5] from the forward rows and d L / d prior."""
    _check_codes(kmer_code)
    n = kmer_code.shape[0]
    for t in (prior, grad_prior):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (n, 5)):
            raise ValueError("prior and grad_prior must be contiguous CUDA float64 tensors [n, 5]")
    ws = ws or default_workspace(kmer_code.device)
    grad = torch.empty((lag, 5, 5), dtype=torch.float64, device=kmer_code.device)
    _launch(kmer_code.device, "bear_linear_backward_f64", ws.handle, _ptr(kmer_code), n, int(lag), _ptr(prior), _ptr(grad_prior),
            _ptr(grad))
    return grad


def _check_codes_wide(codes, lag):
    if not (codes.is_cuda and codes.dtype == torch.int8 and codes.dim() == 2 and codes.shape[1] == lag and codes.is_contiguous()):
        raise ValueError("codes must be a contiguous CUDA int8 tensor [n, lag]")
    if codes.data_ptr() % 16:
        codes = codes.clone()
    return codes


def linear_forward_wide(codes, mat, lag, ws=None):
    """One launch of ``bear_linear_forward_wide_f64``: the rows softmax(sum_l mat[l, codes[l], :]) [n, 21] of protein contexts
    (int8 codes: 0..19 residues, 20 = '[', -1 = unknown letter)."""
    W = LINEAR_WIDE_WIDTH
    codes = _check_codes_wide(codes, lag)
    if not (mat.is_cuda and mat.dtype == torch.float64 and mat.is_contiguous() and tuple(mat.shape) == (lag, W, W)):
        raise ValueError(f"mat must be a contiguous CUDA float64 tensor [lag, {W}, {W}]")
    n = codes.shape[0]
    ws = ws or default_workspace(codes.device)
    prior = torch.empty((n, W), dtype=torch.float64, device=codes.device)
    _launch(codes.device, "bear_linear_forward_wide_f64", ws.handle, _ptr(codes), n, int(lag), W, _ptr(mat), _ptr(prior))
    return prior


def linear_backward_wide(codes, lag, prior, grad_prior, ws=None):
    """One launch of ``bear_linear_backward_wide_f64``: d L / d mat [lag, 21, 21] from the forward rows and d L / d prior.  No
    floating-point atomics: the same inputs give the same bits."""
    W = LINEAR_WIDE_WIDTH
    codes = _check_codes_wide(codes, lag)
    n = codes.shape[0]
    prior = _check_rows(prior, torch.float64, "prior", W)
    grad_prior = _check_rows(grad_prior, torch.float64, "grad_prior", W)
    if prior.shape[0] != n or grad_prior.shape[0] != n:
        raise ValueError("codes, prior and grad_prior must have the same number of rows")
    ws = ws or default_workspace(codes.device)
    grad = torch.empty((lag, W, W), dtype=torch.float64, device=codes.device)
    _launch(codes.device, "bear_linear_backward_wide_f64", ws.handle, _ptr(codes), n, int(lag), W, _ptr(prior), _ptr(grad_prior),
            _ptr(grad))
    return grad


def cnn_param_count_wide(lag, filter_width):
    return _count("bear_cnn_param_count_wide", int(lag), int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, LINEAR_WIDE_WIDTH)


def _check_params_wide(flat_params, lag, filter_width):
    if not (flat_params.is_cuda and flat_params.dtype == torch.float64 and flat_params.dim() == 1 and flat_params.is_contiguous()
            and flat_params.numel() == cnn_param_count_wide(lag, filter_width)):
        raise ValueError("flat_params must be the contiguous CUDA float64 parameter vector of bear_cnn_param_count_wide elements")


def cnn_forward_wide(codes, flat_params, lag, filter_width, save=True, ws=None):
    """One launch of ``bear_cnn_forward_wide_f64``: (prior [n, 21], t1 [n, 16] or None) of protein contexts (int8 codes: 0..19
    residues, 20 = '[', -1 = unknown letter)."""
    W = LINEAR_WIDE_WIDTH
    codes = _check_codes_wide(codes, lag)
    _check_params_wide(flat_params, lag, filter_width)
    n = codes.shape[0]
    ws = ws or default_workspace(codes.device)
    prior = torch.empty((n, W), dtype=torch.float64, device=codes.device)
    t1 = torch.empty((n, CNN_LAYER1_WIDTH), dtype=torch.float64, device=codes.device) if save else None
    _launch(codes.device, "bear_cnn_forward_wide_f64", ws.handle, _ptr(codes), n, int(lag), int(filter_width), CNN_NUM_FILTERS,
            CNN_LAYER1_WIDTH, W, _ptr(flat_params), _ptr(prior), _ptr(t1))
    return prior, t1


def cnn_backward_wide(codes, flat_params, lag, filter_width, t1, prior, grad_prior, ws=None):
    """One launch of ``bear_cnn_backward_wide_f64``: d L / d flat_params from the forward rows, the kept layer-1 sums and
    d L / d prior.  No floating-point atomics: the same inputs give the same bits."""
    W = LINEAR_WIDE_WIDTH
    codes = _check_codes_wide(codes, lag)
    _check_params_wide(flat_params, lag, filter_width)
    n = codes.shape[0]
    prior = _check_rows(prior, torch.float64, "prior", W)
    grad_prior = _check_rows(grad_prior, torch.float64, "grad_prior", W)
    if not (t1.is_cuda and t1.dtype == torch.float64 and t1.dim() == 2 and t1.shape[1] == CNN_LAYER1_WIDTH and t1.is_contiguous()):
        raise ValueError("t1 must be a contiguous CUDA float64 tensor [n, 16] (cnn_forward_wide with save=True)")
    if t1.data_ptr() % 16:
        t1 = t1.clone()
    if prior.shape[0] != n or grad_prior.shape[0] != n or t1.shape[0] != n:
        raise ValueError("codes, t1, prior and grad_prior must have the same number of rows")
    ws = ws or default_workspace(codes.device)
    grad = torch.empty_like(flat_params)
    _launch(codes.device, "bear_cnn_backward_wide_f64", ws.handle, _ptr(codes), n, int(lag), int(filter_width), CNN_NUM_FILTERS,
            CNN_LAYER1_WIDTH, W, _ptr(flat_params), _ptr(t1), _ptr(prior), _ptr(grad_prior), _ptr(grad))
    return grad


def _check_scalar_param(**tensors):
    for name, t in tensors.items():
        if not (t.is_cuda and t.dtype == torch.float64 and t.numel() == 1):
            raise ValueError(f"{name} must be a CUDA float64 tensor of one element")


def ref_mix_forward(net_rows, ref_rows, tau_signed, net_weight_signed, ws=None):
    """One launch of ``bear_ref_mix_forward_f64``: (nw net_rows + jukes_cantor(ref_rows, tau)) / (nw + 1) (bear_ref.py:63-68)."""
    n = net_rows.shape[0]
    for name, t in (("net_rows", net_rows), ("ref_rows", ref_rows)):
        _check_rows(t, torch.float64, name, n=n, clone=False)
    _check_scalar_param(tau_signed=tau_signed, net_weight_signed=net_weight_signed)
    ws = ws or default_workspace(net_rows.device)
    prior = torch.empty_like(net_rows)
    _launch(net_rows.device, "bear_ref_mix_forward_f64", ws.handle, _ptr(net_rows), _ptr(ref_rows), n, _ptr(tau_signed),
            _ptr(net_weight_signed), _ptr(prior))
    return prior


def ref_mix_backward(net_rows, ref_rows, grad_prior, tau_signed, net_weight_signed, ws=None):
    """One launch of ``bear_ref_mix_backward_f64``: (d L / d net_rows [n, 5], [d L / d tau_signed, d L / d net_weight_signed])."""
    n = net_rows.shape[0]
    for name, t in (("net_rows", net_rows), ("ref_rows", ref_rows), ("grad_prior", grad_prior)):
        _check_rows(t, torch.float64, name, n=n, clone=False)
    _check_scalar_param(tau_signed=tau_signed, net_weight_signed=net_weight_signed)
    ws = ws or default_workspace(net_rows.device)
    grad_rows = torch.empty_like(net_rows)
    scalars = torch.empty(2, dtype=torch.float64, device=net_rows.device)
    _launch(net_rows.device, "bear_ref_mix_backward_f64", ws.handle, _ptr(net_rows), _ptr(ref_rows), _ptr(grad_prior), n, _ptr(tau_signed),
            _ptr(net_weight_signed), _ptr(grad_rows), _ptr(scalars))
    return grad_rows, scalars


def stream_read(t, ws=None):
    """One launch of ``bear_stream_read`` over tensor ``t`` (measurement helper: a pure HBM read)."""
    ws = ws or default_workspace(t.device)
    _launch(t.device, "bear_stream_read", ws.handle, _ptr(t), t.numel() * t.element_size())


def encode_kmers(ascii_kmers, alphabet="dna"):
    """One launch of ``bear_encode_kmers_i8``: device uint8 [n, lag] ASCII k-mers -> int8 letter codes [n, lag]
    (the device twin of ``core.encode_kmers``); ``'prot'``: 0..19 residues, 20 = '[', -1 = anything else."""
    if not (ascii_kmers.is_cuda and ascii_kmers.dtype == torch.uint8 and ascii_kmers.dim() == 2 and ascii_kmers.is_contiguous()):
        raise ValueError("ascii_kmers must be a contiguous CUDA uint8 tensor [n, lag]")
    mode = {"dna": 0, "rna": 1, "prot": 2}.get(alphabet)
    if mode is None:
        raise NotImplementedError(f"device encoding covers the alphabets dna, rna and prot, not {alphabet!r}")
    codes = torch.empty(ascii_kmers.shape, dtype=torch.int8, device=ascii_kmers.device)
    _launch(ascii_kmers.device, "bear_encode_kmers_i8", _ptr(ascii_kmers), ascii_kmers.shape[0], ascii_kmers.shape[1], mode, _ptr(codes))
    return codes


def _f64_vec(t, n, name):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{name} must be a contiguous CUDA float64 tensor of {n} elements")


def _loss(loss_buf):
    """(loss_buf, loss_cap) of the step entries: the record of the losses and its length, or NULL and 0."""
    return _ptr(loss_buf), 0 if loss_buf is None else loss_buf.numel()


def dm_prior_planned_dev(plan, prior, h_signed_dev, eps=EPSILON, out=None, normalized=False, want_grad=False, train_ar=False):
    """``bear_dm_prior_plan_dev_f64``: dm_prior_planned with h_signed read from a device tensor, so a training step is
    enqueued without the host reading the parameter back.  Returns out, or (out, grad rows) with want_grad."""
    counts = plan.counts
    _check_planned(plan, 5, prior, torch.float64, "prior")
    _f64_vec(h_signed_dev, 1, "h_signed_dev")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    grad = torch.empty_like(prior) if want_grad else None
    _launch(counts.device, "bear_dm_prior_plan_dev_f64", _step_ws(plan).handle, plan._h, _ptr(counts), _ptr(prior), counts.shape[0],
            _ptr(h_signed_dev), float(eps), int(bool(train_ar)), int(bool(normalized)), _ptr(out), _ptr(grad))
    return (out, grad) if want_grad else out


def dm_refmix_planned_dev(plan, net_rows, ref_rows, h_signed_dev, tau_signed_dev, net_weight_signed_dev, eps=EPSILON, out=None,
                          train_ar=False):
    """``bear_dm_refmix_plan_grad_f64``: bear_ref's step for a net function with parameters, the reference mixing inside the DM step.
    Returns (out [4] = sum LL, d/dh_signed, d/dtau_signed, d/dnet_weight_signed; d sum LL / d net_rows [n, 5])."""
    counts = plan.counts
    n = counts.shape[0]
    for name, t in (("net_rows", net_rows), ("ref_rows", ref_rows)):
        _check_rows(t, torch.float64, name, n=n, clone=False)
    if plan.ncol != 5:
        raise ValueError("a five-column plan of the training counts is needed")
    _check_scalar_param(h_signed_dev=h_signed_dev, tau_signed_dev=tau_signed_dev, net_weight_signed_dev=net_weight_signed_dev)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=counts.device)
    _f64_vec(out, 4, "out")
    grad = torch.empty_like(net_rows)
    _launch(counts.device, "bear_dm_refmix_plan_grad_f64", _step_ws(plan).handle, plan._h, _ptr(counts), _ptr(net_rows), _ptr(ref_rows), n,
            _ptr(h_signed_dev), _ptr(tau_signed_dev), _ptr(net_weight_signed_dev), float(eps), int(bool(train_ar)), _ptr(out), _ptr(grad))
    return out, grad


def train_apply(theta, packed, adam_m, adam_v, adam_t, learning_rate, scale, loss_buf=None, train_ar=False):
    """Enqueues ``bear_train_apply_f64``: tf.keras Adam on ``theta`` with the gradients ``scale * packed[1:]``;
    ``loss_buf[step] = -scale * packed[0]``.  packed = [sum LL, d/d theta...] (after the all-reduce when rows are sharded)."""
    n = theta.numel()
    for t, k, name in ((theta, n, "theta"), (packed, n + 1, "packed"), (adam_m, n, "adam_m"), (adam_v, n, "adam_v"), (adam_t, 1, "adam_t")):
        _f64_vec(t, k, name)
    _launch(theta.device, "bear_train_apply_f64", _ptr(theta), n, _ptr(packed), _ptr(adam_m), _ptr(adam_v), _ptr(adam_t),
            float(learning_rate), float(scale), int(bool(train_ar)), *_loss(loss_buf))


def ref_train_reduce(plan, ref, theta, packed, eps=EPSILON, train_ar=False):
    """Enqueues ``bear_ref_train_reduce_f64``: this shard's packed = [sum LL, d/dh_s, d/dtau_s, d/dnu_s] with the kernel constants
    derived from the device-resident theta (no host round trip)."""
    train = plan.counts
    _check_planned(plan, 4, ref, torch.int32, "ref")
    _f64_vec(theta, 3, "theta")
    _f64_vec(packed, 4, "packed")
    _launch(train.device, "bear_ref_train_reduce_f64", _step_ws(plan).handle, plan._h, _ptr(train), _ptr(ref), train.shape[0], _ptr(theta),
            float(eps), int(bool(train_ar)), _ptr(packed))


def ref_train_step(plan, ref, theta, adam_m, adam_v, adam_t, learning_rate, scale, out, loss_buf=None, eps=EPSILON, train_ar=False):
    """Enqueues one ``bear_ref_train_step_f64`` (constants from theta, planned mode-R kernel, finalize, Adam on theta): no host
    synchronisation, every argument device-resident -- capturable in a HIP graph (``torch.cuda.graph``)."""
    train = plan.counts
    _check_planned(plan, 4, ref, torch.int32, "ref")
    for t, n, name in ((theta, 3, "theta"), (adam_m, 3, "adam_m"), (adam_v, 3, "adam_v"), (adam_t, 1, "adam_t"), (out, 4, "out")):
        _f64_vec(t, n, name)
    _launch(train.device, "bear_ref_train_step_f64", _step_ws(plan).handle, plan._h, _ptr(train), _ptr(ref), train.shape[0], _ptr(theta),
            _ptr(adam_m), _ptr(adam_v), _ptr(adam_t), float(eps), int(bool(train_ar)), float(learning_rate), float(scale), _ptr(out),
            *_loss(loss_buf))


def _check_linear_step(plan, kmer_code, lag, theta, packed):
    n = plan.counts.shape[0]
    _f64_vec(theta, 1 + lag * 25, "theta")
    _f64_vec(packed, 2 + lag * 25, "packed")
    if not (kmer_code.is_cuda and kmer_code.dtype == torch.int64 and kmer_code.is_contiguous() and kmer_code.shape == (n,)
            and kmer_code.data_ptr() % 16 == 0):
        raise ValueError("kmer_index must be a contiguous, 16-byte aligned CUDA int64 tensor [n_rows] (linear_index)")
    return n


def net_linear_train_reduce(plan, kmer_code, lag, theta, packed, eps=EPSILON, train_ar=False):
    """Enqueues ``bear_net_linear_train_reduce_f64``: packed = [sum LL, d/dh_s, d/d mat (lag*25)] of this shard, theta = {h_signed, mat}
    device-resident."""
    n = _check_linear_step(plan, kmer_code, lag, theta, packed)
    _launch(theta.device, "bear_net_linear_train_reduce_f64", _step_ws(plan).handle, plan._h, _ptr(plan.counts), _ptr(kmer_code), int(lag), n,
            _ptr(theta), float(eps), int(bool(train_ar)), _ptr(packed))


def net_linear_train_step(plan, kmer_code, lag, theta, adam_m, adam_v, adam_t, packed, learning_rate, scale, loss_buf=None,
                          eps=EPSILON, train_ar=False):
    """Enqueues one ``bear_net_linear_train_step_f64`` (HIP-graph capturable): theta = {h_signed, mat} on the device."""
    n = _check_linear_step(plan, kmer_code, lag, theta, packed)
    size = 1 + lag * 25
    for t, k in ((adam_m, size), (adam_v, size), (adam_t, 1)):
        _f64_vec(t, k, "adam state")
    _launch(theta.device, "bear_net_linear_train_step_f64", _step_ws(plan).handle, plan._h, _ptr(plan.counts), _ptr(kmer_code), int(lag), n,
            _ptr(theta), _ptr(adam_m), _ptr(adam_v), _ptr(adam_t), _ptr(packed), float(eps), int(bool(train_ar)), float(learning_rate),
            float(scale), *_loss(loss_buf))


# tile and resident blocks per CU of the fused linear step at width 21 (kernels_linear_wide.h: LSW_TILE, LSW_BLOCKS_PER_CU): a launch
# takes min(tiles, blocks per CU * CUs) blocks -- tests size a table beyond that from these
LINEAR_STEP_WIDE_TILE = 128
LINEAR_STEP_WIDE_BLOCKS_PER_CU = 2


def _check_linear_step_wide(counts, codes, lag):
    W = LINEAR_WIDE_WIDTH
    if not 1 <= int(lag) <= LINEAR_WIDE_MAX_LAG:
        raise ValueError(f"lag must be 1..{LINEAR_WIDE_MAX_LAG} (mat [lag, {W}, {W}] lives in LDS)")
    counts, codes = _check_rows(counts, torch.int32, "counts", W), _check_codes_wide(codes, lag)
    if codes.shape[0] != counts.shape[0] or codes.device != counts.device:
        raise ValueError("counts and codes must have the same number of rows, on one device")
    return counts, codes


def dm_linear_wide(counts, codes, mat, h_signed, eps=EPSILON, train_ar=False, out=None, ws=None):
    """One launch of ``bear_dm_linear_wide_f64``: ``dm_linear`` on protein rows without a plan -- the linear AR function, the DM step
    and the gradient of mat in one kernel (what ``linear_forward_wide``, ``dm_prior_wide(want_grad=True)`` and ``linear_backward_wide``
    compute in three).  Returns (out [2] = sum LL, d/dh_signed; d sum LL / d mat [lag, 21, 21])."""
    W = LINEAR_WIDE_WIDTH
    if not (mat.dim() == 3 and tuple(mat.shape[1:]) == (W, W)):
        raise ValueError(f"mat must be a contiguous CUDA float64 tensor [lag, {W}, {W}]")
    lag = mat.shape[0]
    counts, codes = _check_linear_step_wide(counts, codes, lag)
    if not (mat.is_cuda and mat.dtype == torch.float64 and mat.is_contiguous() and mat.device == counts.device):
        raise ValueError(f"mat must be a contiguous CUDA float64 tensor [lag, {W}, {W}]")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    _f64_vec(out, 2, "out")
    ws = ws or default_workspace(counts.device)
    grad = torch.empty_like(mat)
    _launch(counts.device, "bear_dm_linear_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag), W, _ptr(mat),
            float(h_signed), float(eps), int(bool(train_ar)), _ptr(out), _ptr(grad))
    return out, grad


def net_linear_train_reduce_wide(counts, codes, lag, theta, packed, eps=EPSILON, train_ar=False, ws=None):
    """Enqueues ``bear_net_linear_train_reduce_wide_f64``: packed = [sum LL, d/dh_s, d/d mat (lag*441)] of these rows, theta =
    {h_signed, mat} device-resident."""
    counts, codes = _check_linear_step_wide(counts, codes, lag)
    size = 1 + lag * LINEAR_WIDE_WIDTH * LINEAR_WIDE_WIDTH
    _f64_vec(theta, size, "theta")
    _f64_vec(packed, size + 1, "packed")
    ws = ws or default_workspace(counts.device)
    _launch(counts.device, "bear_net_linear_train_reduce_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag),
            LINEAR_WIDE_WIDTH, _ptr(theta), float(eps), int(bool(train_ar)), _ptr(packed))


def net_linear_train_step_wide(counts, codes, lag, theta, adam_m, adam_v, adam_t, packed, learning_rate, scale, loss_buf=None,
                               eps=EPSILON, train_ar=False, ws=None):
    """Enqueues one ``bear_net_linear_train_step_wide_f64`` (HIP-graph capturable): the reduce and tf.keras Adam on theta =
    {h_signed, mat [lag, 21, 21]} in one launch."""
    counts, codes = _check_linear_step_wide(counts, codes, lag)
    size = 1 + lag * LINEAR_WIDE_WIDTH * LINEAR_WIDE_WIDTH
    for t, k, name in ((theta, size, "theta"), (adam_m, size, "adam_m"), (adam_v, size, "adam_v"), (adam_t, 1, "adam_t"),
                       (packed, size + 1, "packed")):
        _f64_vec(t, k, name)
    if loss_buf is not None:
        _f64_vec(loss_buf, loss_buf.numel(), "loss_buf")
    ws = ws or default_workspace(counts.device)
    _launch(counts.device, "bear_net_linear_train_step_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag),
            LINEAR_WIDE_WIDTH, _ptr(theta), _ptr(adam_m), _ptr(adam_v), _ptr(adam_t), float(eps), int(bool(train_ar)), float(learning_rate),
            float(scale), _ptr(packed), *_loss(loss_buf))


_CNN_RESERVATION = "the convolutional step's reservation (cnn_step_buffers)"


def net_cnn_train_reduce(plan, kmer_code, lag, filter_width, theta, bufs, packed, eps=EPSILON, train_ar=False):
    """Enqueues ``bear_net_cnn_train_reduce_f64``: forward, planned DM kernel with gradient rows, backward;
    packed = [sum LL, d/dh_s, d/d params] of this shard.  ``bufs`` = (prior [n,5], t1 [n,16], grad_rows [n,5]) from ``cnn_step_buffers``.
    The reservation lives in ``plan.ws``: the step runs on the stream that workspace belongs to (``_step_ws``; ValueError otherwise)."""
    n = plan.counts.shape[0]
    prior, t1, grad_rows = bufs
    np_ = cnn_param_count(lag, filter_width)
    _f64_vec(theta, 1 + np_, "theta")
    _f64_vec(packed, 2 + np_, "packed")
    _launch(theta.device, "bear_net_cnn_train_reduce_f64", _step_ws(plan, owns=_CNN_RESERVATION).handle, plan._h, _ptr(plan.counts), _ptr(kmer_code), n, int(lag),
            int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, _ptr(theta), _ptr(prior), _ptr(t1), _ptr(grad_rows), float(eps),
            int(bool(train_ar)), _ptr(packed))


def net_cnn_train_step(plan, kmer_code, lag, filter_width, theta, adam_m, adam_v, adam_t, bufs, packed, learning_rate, scale, loss_buf=None,
                       eps=EPSILON, train_ar=False):
    """Enqueues one ``bear_net_cnn_train_step_f64`` (HIP-graph capturable): theta = {h_signed, flat CNN parameters} on the device;
    ``bufs`` = (prior [n,5], t1 [n,16], grad_rows [n,5]) lent by the caller (``cnn_step_buffers``).  Like the reduce, on the stream
    that owns ``plan.ws`` only."""
    n = plan.counts.shape[0]
    prior, t1, grad_rows = bufs
    np_ = cnn_param_count(lag, filter_width)
    _f64_vec(theta, 1 + np_, "theta")
    _f64_vec(packed, 2 + np_, "packed")
    _launch(theta.device, "bear_net_cnn_train_step_f64", _step_ws(plan, owns=_CNN_RESERVATION).handle, plan._h, _ptr(plan.counts), _ptr(kmer_code), n, int(lag),
            int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, _ptr(theta), _ptr(adam_m), _ptr(adam_v), _ptr(adam_t), _ptr(prior),
            _ptr(t1), _ptr(grad_rows), _ptr(packed), float(eps), int(bool(train_ar)), float(learning_rate), float(scale), *_loss(loss_buf))


def cnn_step_buffers(n_rows, lag, filter_width, device, ws=None):
    """Per-context scratch of the CNN step for (at most) ``n_rows`` contexts + the library-side reservation (``bear_cnn_reserve``):
    (prior [n,5], t1 [n,16], grad_rows [n,5]).  Steps on one stream run one after the other, so one set sized for the largest
    batch serves every batch."""
    ws = ws or default_workspace(device)
    with torch.cuda.device(device):
        _lib.call("bear_cnn_reserve", ws.handle, int(n_rows), int(lag), int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH)
    # zeros: the step only fills the rows of contexts that hold training counts (nothing reads the others: kept finite)
    return (torch.zeros((n_rows, 5), dtype=torch.float64, device=device), torch.zeros((n_rows, CNN_LAYER1_WIDTH), dtype=torch.float64, device=device),
            torch.zeros((n_rows, 5), dtype=torch.float64, device=device))


# tiles and resident blocks per CU of the two launches of the convolutional step at width 21 (kernels_cnn_wide.h: CNW_HEAD_TILE,
# CNW_HEAD_BLOCKS_PER_CU; CNW_BWD_TILE, CNW_BWD_BLOCKS_PER_CU): each takes min(tiles, blocks per CU * CUs) blocks, and each grid is
# part of the result -- tests size a table beyond both from these
CNN_STEP_WIDE_TILE = 256
CNN_STEP_WIDE_BLOCKS_PER_CU = 1
CNN_STEP_WIDE_BACKWARD_TILE = 64
CNN_STEP_WIDE_BACKWARD_BLOCKS_PER_CU = 1


def cnn_step_buffers_wide(n_rows, device):
    """Per-context scratch of the convolutional step at width 21 for (at most) ``n_rows`` contexts: (dz [n, 21], t1 [n, 16]), 296 B
    per context.  Steps on one stream run one after the other, so one pair sized for the largest batch serves every batch."""
    n = max(int(n_rows), 1)
    return (torch.zeros((n, LINEAR_WIDE_WIDTH), dtype=torch.float64, device=device),
            torch.zeros((n, CNN_LAYER1_WIDTH), dtype=torch.float64, device=device))


def _check_cnn_step_wide(counts, codes, lag, filter_width, bufs):
    """The shape checks of the three entries; returns (counts, codes, dz, t1, parameter count)."""
    if not cnn_supported(int(lag), 20, int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH):
        raise ValueError(f"1 <= filter_width <= lag <= {CNN_WIDE_MAX_LAG} (the filter image and a tile's staged rows live in LDS)")
    counts, codes = _check_rows(counts, torch.int32, "counts", LINEAR_WIDE_WIDTH), _check_codes_wide(codes, lag)
    if codes.shape[0] != counts.shape[0] or codes.device != counts.device:
        raise ValueError("counts and codes must have the same number of rows, on one device")
    n = counts.shape[0]
    dz, t1 = bufs if bufs is not None else cnn_step_buffers_wide(n, counts.device)
    for t, w, name in ((dz, LINEAR_WIDE_WIDTH, "dz"), (t1, CNN_LAYER1_WIDTH, "t1")):
        if not (t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == w and t.shape[0] >= n and t.is_contiguous()
                and t.data_ptr() % 16 == 0 and t.device == counts.device):
            raise ValueError(f"bufs: {name} must be a contiguous, 16-byte aligned CUDA float64 tensor [>= n_rows, {w}] (cnn_step_buffers_wide)")
    return counts, codes, dz, t1, cnn_param_count_wide(lag, filter_width)


def dm_cnn_wide(counts, codes, flat_params, lag, filter_width, h_signed, eps=EPSILON, train_ar=False, bufs=None, out=None, ws=None):
    """``bear_dm_cnn_wide_f64``: the convolutional AR function, the DM step and the gradient of the parameters on protein rows in two
    launches (what ``cnn_forward_wide``, ``dm_prior_wide(want_grad=True)`` and ``cnn_backward_wide`` compute in three, with the row
    arrays through memory).  ``bufs``: ``cnn_step_buffers_wide`` (made here when None).  Returns (out [2] = sum LL, d/dh_signed;
    d sum LL / d flat_params)."""
    counts, codes, dz, t1, np_ = _check_cnn_step_wide(counts, codes, lag, filter_width, bufs)
    _check_params_wide(flat_params, lag, filter_width)
    if flat_params.device != counts.device:
        raise ValueError("flat_params: on another device than counts")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=counts.device)
    _f64_vec(out, 2, "out")
    ws = ws or default_workspace(counts.device)
    grad = torch.empty_like(flat_params)
    _launch(counts.device, "bear_dm_cnn_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag), int(filter_width),
            CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, LINEAR_WIDE_WIDTH, _ptr(flat_params), float(h_signed), float(eps), int(bool(train_ar)),
            _ptr(dz), _ptr(t1), _ptr(out), _ptr(grad))
    return out, grad


def net_cnn_train_reduce_wide(counts, codes, lag, filter_width, theta, bufs, packed, eps=EPSILON, train_ar=False, ws=None):
    """Enqueues ``bear_net_cnn_train_reduce_wide_f64``: packed = [sum LL, d/dh_s, d/d params] of these rows, theta = {h_signed, flat
    CNN parameters} device-resident; ``bufs`` = (dz [n, 21], t1 [n, 16]) from ``cnn_step_buffers_wide``."""
    counts, codes, dz, t1, np_ = _check_cnn_step_wide(counts, codes, lag, filter_width, bufs)
    _f64_vec(theta, 1 + np_, "theta")
    _f64_vec(packed, 2 + np_, "packed")
    ws = ws or default_workspace(counts.device)
    _launch(counts.device, "bear_net_cnn_train_reduce_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag),
            int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, LINEAR_WIDE_WIDTH, _ptr(theta), _ptr(dz), _ptr(t1), float(eps),
            int(bool(train_ar)), _ptr(packed))


def net_cnn_train_step_wide(counts, codes, lag, filter_width, theta, adam_m, adam_v, adam_t, bufs, packed, learning_rate, scale,
                            loss_buf=None, eps=EPSILON, train_ar=False, ws=None):
    """Enqueues one ``bear_net_cnn_train_step_wide_f64`` (HIP-graph capturable): the reduce and tf.keras Adam on theta = {h_signed,
    flat CNN parameters}, the update in the block of the second launch that sums the gradient."""
    counts, codes, dz, t1, np_ = _check_cnn_step_wide(counts, codes, lag, filter_width, bufs)
    for t, k, name in ((theta, 1 + np_, "theta"), (adam_m, 1 + np_, "adam_m"), (adam_v, 1 + np_, "adam_v"), (adam_t, 1, "adam_t"),
                       (packed, 2 + np_, "packed")):
        _f64_vec(t, k, name)
    if loss_buf is not None:
        _f64_vec(loss_buf, loss_buf.numel(), "loss_buf")
    ws = ws or default_workspace(counts.device)
    _launch(counts.device, "bear_net_cnn_train_step_wide_f64", ws.handle, _ptr(counts), _ptr(codes), counts.shape[0], int(lag),
            int(filter_width), CNN_NUM_FILTERS, CNN_LAYER1_WIDTH, LINEAR_WIDE_WIDTH, _ptr(theta), _ptr(adam_m), _ptr(adam_v), _ptr(adam_t),
            _ptr(dz), _ptr(t1), float(eps), int(bool(train_ar)), float(learning_rate), float(scale), _ptr(packed), *_loss(loss_buf))
