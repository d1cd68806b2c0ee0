"""bear_net's convolutional step at the protein alphabet's width without a device: both builds export the three symbols under the
unchanged ABI version, the binding declares them with the header's argument lists, without a device they answer BEAR_ERR_NO_DEVICE,
the geometry constants are the header's, and bear_net.step_form selects the path exactly where it should."""
import ctypes
import os
import re

import pytest
import torch

from bear_amd import _lib, _train, ar_funcs, bear_net, kernels
from conftest import ROOT
from util import abi_header

NEW = ["bear_dm_cnn_wide_f64", "bear_net_cnn_train_reduce_wide_f64", "bear_net_cnn_train_step_wide_f64"]
W = 21


def test_both_builds_export_the_symbols_at_abi_12():
    L = _lib.lib()
    version, sigs = abi_header()
    assert _lib.ABI_VERSION == 12 and L.bear_abi_version() == 12 and version == 12
    det = ctypes.CDLL(os.path.join(ROOT, "bear_amd", "libbear_hip_det.so"))
    assert det.bear_abi_version() == 12
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name) and hasattr(det, name), name
        assert sigs[name][0] is ctypes.c_int and list(getattr(L, name).argtypes) == sigs[name][1], name
    vp, u64, i32, f64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
    shape = [vp, vp, vp, u64, i32, i32, i32, i32, i32]          # ws, counts, codes, n_rows, lag, fw, nf, l1, width
    assert list(L.bear_dm_cnn_wide_f64.argtypes) == shape + [vp, f64, f64, i32, vp, vp, vp, vp, vp]
    assert list(L.bear_net_cnn_train_reduce_wide_f64.argtypes) == shape + [vp, vp, vp, f64, i32, vp, vp]
    assert list(L.bear_net_cnn_train_step_wide_f64.argtypes) == shape + [vp, vp, vp, vp, vp, vp, f64, i32, f64, f64, vp, vp, u64, vp]


def test_tile_constants_are_the_headers():
    src = open(os.path.join(ROOT, "bear_amd", "csrc", "kernels_cnn_wide.h")).read()

    def define(name):
        v = re.search(r"#define %s\s+(\w+)" % name, src).group(1)
        return int(v) if v.isdigit() else define(v)
    assert kernels.CNN_STEP_WIDE_TILE == define("CNW_HEAD_TILE")
    assert kernels.CNN_STEP_WIDE_BLOCKS_PER_CU == define("CNW_HEAD_BLOCKS_PER_CU")
    assert kernels.CNN_STEP_WIDE_BACKWARD_TILE == define("CNW_BWD_TILE")
    assert kernels.CNN_STEP_WIDE_BACKWARD_BLOCKS_PER_CU == define("CNW_BWD_BLOCKS_PER_CU")


def test_no_device_is_a_loud_error():
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    L = _lib.lib()
    ws = ctypes.create_string_buffer(4096)                       # (never read: the entries ask for the device first)
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)
    shape = (ws, p, p, 8, 4, 2, 30, 16, W)
    assert L.bear_dm_cnn_wide_f64(*shape, p, 0.0, 1e-7, 0, p, p, p, p, None) == -2          # BEAR_ERR_NO_DEVICE
    assert L.bear_net_cnn_train_reduce_wide_f64(*shape, p, p, p, 1e-7, 0, p, None) == -2
    assert L.bear_net_cnn_train_step_wide_f64(*shape, p, p, p, p, p, p, 1e-7, 0, 0.01, 1.0, p, None, 0, None) == -2
    # a refused shape is refused first
    assert L.bear_dm_cnn_wide_f64(ws, p, p, 8, 4, 2, 30, 16, 5, p, 0.0, 1e-7, 0, p, p, p, p, None) == -1
    with pytest.raises(ValueError):
        kernels.dm_cnn_wide(torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 4), dtype=torch.int8), torch.zeros(10, dtype=torch.float64),
                            4, 2, 0.0)


def _form(ar_func, params, alphabet_size, lag, width):
    return bear_net.step_form(ar_func, params, alphabet_size, lag, width)[0]


def test_step_form_selects_cnn_wide(monkeypatch):
    """The test that fails without the feature: the convolutional AR function on a protein table has a fused form."""
    monkeypatch.delenv("BEAR_AMD_UNFUSED_CNN_WIDE", raising=False)
    f, params = ar_funcs.make_ar_func_cnn(12, 20, filter_width=8)
    form, kw = bear_net.step_form(f, params, 20, 12, W)
    assert form == "cnn_wide"
    assert kw["kmer_order"] is False and kw["prebuild"] == [("train", _train.ROWS_IF_DENSE, None)]
    assert kw["per_row_extra"] == 8 * (21 + 16)                  # the dz and t1 rows of the one buffer pair: 296 B
    monkeypatch.setenv("BEAR_AMD_UNFUSED_CNN_WIDE", "0")
    assert _form(f, params, 20, 12, W) == "cnn_wide"
    monkeypatch.setenv("BEAR_AMD_UNFUSED_CNN_WIDE", "1")
    assert _form(f, params, 20, 12, W) is None
    monkeypatch.delenv("BEAR_AMD_UNFUSED_CNN_WIDE")
    assert _form(f, params, 20, 12, 5) is None                   # a 5-wide table
    assert _form(f, list(params), 20, 12, W) == "cnn_wide"       # (another list of the same tensors)
    assert _form(f, [p.detach().clone().requires_grad_(True) for p in params], 20, 12, W) is None      # equal, not identical
    assert _form(f, params[:7], 20, 12, W) is None
    f17, p17 = ar_funcs.make_ar_func_cnn(17, 20, filter_width=8)
    assert _form(f17, p17, 20, 17, W) is None                    # beyond CNN_WIDE_MAX_LAG
    f20, p20 = ar_funcs.make_ar_func_cnn(12, 20, filter_width=8, num_filters=20)
    assert _form(f20, p20, 20, 12, W) is None                    # 20 filters: the torch formulation
    for lag, fw in ((1, 1), (16, 16), (16, 1)):
        g, q = ar_funcs.make_ar_func_cnn(lag, 20, filter_width=fw)
        assert _form(g, q, 20, lag, W) == "cnn_wide"


def test_the_other_forms_are_unchanged(monkeypatch):
    monkeypatch.delenv("BEAR_AMD_UNFUSED_CNN_WIDE", raising=False)
    monkeypatch.delenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", raising=False)
    f4, p4 = ar_funcs.make_ar_func_cnn(12, 4, filter_width=8)
    form, kw = bear_net.step_form(f4, p4, 4, 12, 5)
    assert form == "cnn" and kw["kmer_order"] is True and kw["per_row_extra"] == 8 + 208 + 64
    fl, pl = ar_funcs.make_ar_func_linear(4, 20)
    form, kw = bear_net.step_form(fl, pl, 20, 4, W)
    assert form == "linear_wide" and kw["per_row_extra"] == 0
    fl4, pl4 = ar_funcs.make_ar_func_linear(4, 4)
    assert _form(fl4, pl4, 4, 4, 5) == "linear"
    fs, ps = ar_funcs.make_ar_func_stop(4, 20)
    form, kw = bear_net.step_form(fs, ps, 20, 4, W)
    assert form is None and kw["per_row_extra"] == 16 * 21
