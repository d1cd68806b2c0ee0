"""bear_ref's wide entries without a device: the wrappers refuse wrong shapes, dtypes and widths before any launch, the binding
declares the four symbols with the header's argument lists, and the tile constants tests size their tables from are the header's."""
import ctypes
import os
import re

import pytest
import torch

from bear_amd import _lib, kernels
from conftest import ROOT
from util import abi_header

NEW = ["bear_dm_ref_wide_f64", "bear_ref_train_reduce_wide_f64", "bear_ref_train_step_wide_f64", "bear_dm_refmix_wide_grad_f64"]


def _rows(n, w, dtype):
    return torch.zeros((n, w), dtype=dtype)


def _vec(n, dtype=torch.float64):
    return torch.zeros(n, dtype=dtype)


@pytest.mark.parametrize("train,ref", [
    (_rows(8, 21, torch.int32), _rows(8, 21, torch.int32)),          # right shapes, but no device
    (_rows(8, 7, torch.int32), _rows(8, 7, torch.int32)),            # a width no kernel has
    (_rows(8, 21, torch.int32), _rows(8, 5, torch.int32)),           # two widths
    (_rows(8, 21, torch.int32), _rows(9, 21, torch.int32)),          # two row counts
    (_rows(8, 21, torch.int64), _rows(8, 21, torch.int64)),          # wrong dtype
    (_vec(21, torch.int32), _vec(21, torch.int32)),                  # not rows
])
def test_wrappers_refuse_before_any_launch(train, ref):
    n = train.shape[0]
    theta, m, v, t, out = _vec(3), _vec(3), _vec(3), _vec(1), _vec(4)
    with pytest.raises(ValueError):
        kernels.dm_ref_wide(train, ref, 0.0, -1.0, -1.0)
    with pytest.raises(ValueError):
        kernels.ref_train_reduce_wide(train, ref, theta, out)
    with pytest.raises(ValueError):
        kernels.ref_train_step_wide(train, ref, theta, m, v, t, 0.01, -1.0, out)
    net = torch.zeros((n, train.shape[-1]), dtype=torch.float64)
    with pytest.raises(ValueError):
        kernels.dm_refmix_wide_dev(train, net, ref, _vec(1), _vec(1), _vec(1))
    with pytest.raises(ValueError):
        kernels.dm_refmix_wide_dev(train, net.to(torch.float32), ref, _vec(1), _vec(1), _vec(1))


def test_binding_declares_the_new_symbols():
    L = _lib.lib()
    sigs = abi_header()[1]
    assert _lib.ABI_VERSION == 12 and L.bear_abi_version() == 12
    det = ctypes.CDLL(os.path.join(ROOT, "bear_amd", "libbear_hip_det.so"))
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name) and hasattr(det, name), name
        assert sigs[name][0] is ctypes.c_int and list(getattr(L, name).argtypes) == sigs[name][1], name


def test_tile_constants_are_the_headers():
    src = open(os.path.join(ROOT, "bear_amd", "csrc", "kernels_refmix_wide.h")).read()

    def tiles(macro):
        wide, narrow = re.search(r"#define %s\(W\) \(\(W\) > 8 \? (\d+) : (\d+)\)" % macro, src).groups()
        return {21: int(wide), 5: int(narrow)}

    def number(macro):
        return int(re.search(r"#define %s (\d+)" % macro, src).group(1))
    assert kernels.REF_WIDE_TILE == tiles("RFW_TILE") and kernels.REFMIX_WIDE_TILE == tiles("RMW_TILE")
    assert kernels.REF_WIDE_BLOCKS_PER_CU == number("RFW_BLOCKS_PER_CU") and kernels.REFMIX_WIDE_BLOCKS_PER_CU == number("RMW_BLOCKS_PER_CU")
