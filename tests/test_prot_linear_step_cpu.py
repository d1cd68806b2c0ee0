"""bear_net's fused linear step at the protein alphabet's width without a device: both builds export the three symbols under the
unchanged ABI version, the binding declares them with the header's argument lists, the wrappers refuse wrong dtypes, shapes and
devices before any library call, and bear_net.train's dispatch predicate selects the path exactly where the issue says."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from bear_amd import _lib, bear_net, kernels
from conftest import ROOT
from util import abi_header

NEW = ["bear_dm_linear_wide_f64", "bear_net_linear_train_reduce_wide_f64", "bear_net_linear_train_step_wide_f64"]
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


def test_tile_constants_are_the_headers():
    src = open(os.path.join(ROOT, "bear_amd", "csrc", "kernels_linear_wide.h")).read()
    assert kernels.LINEAR_STEP_WIDE_TILE == int(re.search(r"#define LSW_TILE (\d+)", src).group(1))
    assert kernels.LINEAR_STEP_WIDE_BLOCKS_PER_CU == int(re.search(r"#define LSW_BLOCKS_PER_CU (\d+)", src).group(1))


def _vec(n, dtype=torch.float64):
    return torch.zeros(n, dtype=dtype)


@pytest.mark.parametrize("counts,codes,lag", [
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.int8), 3),          # right shapes, but no device
    (torch.zeros((8, 5), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.int8), 3),          # a width the kernel does not have
    (torch.zeros((8, W), dtype=torch.int64), torch.zeros((8, 3), dtype=torch.int8), 3),          # wrong dtype of the counts
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.int64), 3),         # ... of the codes
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((9, 3), dtype=torch.int8), 3),          # two row counts
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 4), dtype=torch.int8), 3),          # codes of another lag
    (torch.zeros(8 * W, dtype=torch.int32), torch.zeros((8, 3), dtype=torch.int8), 3),           # not rows
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 17), dtype=torch.int8), 17),        # a lag beyond the kernel's
    (torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 0), dtype=torch.int8), 0),
])
def test_wrappers_refuse_before_any_library_call(counts, codes, lag, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(kernels, "default_workspace", lambda *a, **kw: pytest.fail("a workspace was asked for"))
    size = 1 + lag * W * W
    theta, m, v, t, packed = _vec(size), _vec(size), _vec(size), _vec(1), _vec(size + 1)
    with pytest.raises(ValueError):
        kernels.dm_linear_wide(counts, codes, torch.zeros((lag, W, W), dtype=torch.float64), 0.0)
    with pytest.raises(ValueError):
        kernels.net_linear_train_reduce_wide(counts, codes, lag, theta, packed)
    with pytest.raises(ValueError):
        kernels.net_linear_train_step_wide(counts, codes, lag, theta, m, v, t, packed, 0.01, -1.0)


def test_mat_of_another_shape_is_refused():
    counts, codes = torch.zeros((8, W), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.int8)
    for mat in (torch.zeros((3, 5, 5), dtype=torch.float64), torch.zeros((3, W * W), dtype=torch.float64), torch.zeros((3, W, W), dtype=torch.float32)):
        with pytest.raises(ValueError):
            kernels.dm_linear_wide(counts, codes, mat, 0.0)


def test_dispatch_predicate(monkeypatch):
    monkeypatch.delenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", raising=False)
    sel = bear_net.linear_wide_step_selected
    for alphabet_size, lag, own_mat, width in itertools.product((4, 20), (0, 1, 4, 16, 17), (False, True), (5, 21)):
        want = alphabet_size == 20 and 1 <= lag <= 16 and own_mat and width == 21
        assert sel(alphabet_size, lag, own_mat, width) is want, (alphabet_size, lag, own_mat, width)
    monkeypatch.setenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", "1")
    assert sel(20, 4, True, 21) is False
    monkeypatch.setenv("BEAR_AMD_UNFUSED_LINEAR_WIDE", "0")
    assert sel(20, 4, True, 21) is True


class _Stale:
    """A loaded library without the symbols ``missing``."""

    def __init__(self, real, missing):
        self._real, self._missing = real, missing

    def __getattr__(self, name):
        if name in self._missing:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_stale_library_is_named(monkeypatch, tmp_path):
    """A library that answers ABI 12 but was built before the three symbols: the loader names the first one and the rebuild command."""
    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return getattr(self._real, name)
    real = ctypes.CDLL(_lib.LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Stale(real))
    with pytest.raises(ImportError, match=r"bear_dm_linear_wide_f64.*make -C"):
        _lib._load()


@pytest.mark.parametrize("missing", ["bear_ws_destroy", "bear_eval_plan_f64", "bear_cache_read", "bear_write_counts_tsv_wide"])
def test_stale_library_is_named_for_any_declared_symbol(monkeypatch, missing):
    """... and not only for the newest ones: any function the header declares and the library lacks is named."""
    real = ctypes.CDLL(_lib.LIB_PATH)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: _Stale(real, {missing}))
    with pytest.raises(ImportError, match=r"stale.*does not export %s;.*make -C" % missing):
        _lib._load()
