"""CPU tests of the exact sequence marginal on the device (kernels_marg.h, bear_score_marg_f64, get_bear_probs_seqs with
``marg_on_device``): the entry in the header and the binding, its refusals before any device call, and the keyword's refusals."""
import ctypes
import inspect

import numpy as np
import pytest

from util import abi_header

ENTRY = "bear_score_marg_f64"


def test_entry_declared_and_bound():
    from bear_amd import _lib, kernels
    version, sigs = abi_header()
    assert version == 12 == _lib.ABI_VERSION
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    want = [vp, vp, u64, vp, u64, i, vp, vp, u64, vp, i, vp, i, vp, vp]
    assert ENTRY in _lib.SYMBOLS and sigs[ENTRY] == (i, want)
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is i and list(fn.argtypes) == want
    assert callable(kernels.score_marg)
    header = open(_lib.HEADER_PATH).read()
    assert "#define BEAR_MARG_CHUNK %d" % kernels.MARG_CHUNK in header
    assert "#define BEAR_MARG_MAX_MODELS %d" % kernels.MARG_MAX_MODELS in header and kernels.MARG_MAX_MODELS >= 16
    det = ctypes.CDLL(_lib.LIB_PATH.replace("libbear_hip.so", "libbear_hip_det.so"))
    assert hasattr(det, ENTRY)


def _call(width=5, prior=None, K=10, h=(), van=(0.1, 1.0), n_seg=0, n_h=None, n_van=None, rows=None, letters=None, n_t=0, seg=None,
          train=None, scores=None):
    """The entry with host vectors h / van and the given (fake) device addresses: every case here returns before a device call."""
    from bear_amd import _lib
    h, van = np.asarray(h, dtype=np.float64), np.asarray(van, dtype=np.float64)
    return _lib.lib().bear_score_marg_f64(rows, letters, n_t, seg, n_seg, width, train, prior, K,
                                          h.ctypes.data if h.size else None, h.size if n_h is None else n_h,
                                          van.ctypes.data if van.size else None, van.size if n_van is None else n_van, scores, None)


def test_arguments_are_checked_before_any_device_call():
    from bear_amd import kernels
    assert _call() == 0                                               # n_seg == 0: nothing to launch
    assert _call(width=21, h=(0.05, 3.0), prior=0x1000) == 0
    for width in (0, 4, 6, 20, 22):
        assert _call(width=width) == -1
    assert _call(h=(1.0,), prior=None) == -1                          # BEAR models without prior rows
    assert _call(h=(1.0,), prior=0x1000) == 0
    for bad in (0.0, -1.0, float("nan")):
        assert _call(van=(1.0, bad)) == -1
        assert _call(h=(bad, 1.0), prior=0x1000) == -1
    assert _call(van=()) == -1                                        # no model at all
    assert _call(van=np.ones(kernels.MARG_MAX_MODELS)) == 0
    assert _call(van=np.ones(kernels.MARG_MAX_MODELS + 1)) == -1
    assert _call(h=np.ones(kernels.MARG_MAX_MODELS), van=(1.0,), prior=0x1000) == -1
    assert _call(n_h=-1) == -1 and _call(n_van=-1) == -1
    assert _call(K=2 ** 32 - 1) == -1 and _call(K=2 ** 32 - 2) == 0
    # pointers, with a segment to score: missing, then misaligned (addresses that are never followed)
    ok = dict(n_seg=1, n_t=4, rows=0x1000, letters=0x1001, seg=0x2000, train=0x3000, scores=0x4000)
    for name in ("rows", "letters", "seg", "train", "scores"):
        assert _call(**dict(ok, **{name: None})) == -1, name
    for name, address in (("rows", 0x1002), ("seg", 0x2004), ("train", 0x3002), ("scores", 0x4004)):
        assert _call(**dict(ok, **{name: address})) == -1, name
    assert _call(**dict(ok, h=(1.0,), prior=0x5004)) == -1


def test_keyword_and_its_refusals_need_no_device(monkeypatch):
    import torch
    from bear_amd import get_var_probs, kernels
    p = inspect.signature(get_var_probs.get_bear_probs_seqs).parameters["marg_on_device"]
    assert p.default is False
    assert callable(get_var_probs._marg_segments)

    def no_device(*args, **kwargs):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(kernels, "_launch", no_device)
    monkeypatch.setattr(get_var_probs, "_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    kw = dict(vans=[0.1, 1.0], lag=3, alphabet_name="dna", marg_on_device=True)

    def plain_counter(kmers):
        return np.zeros(np.asarray(kmers).shape + (5,))
    with pytest.raises(ValueError, match="marg_on_device"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=plain_counter, get_marg=True, **kw)
    dev = object.__new__(get_var_probs.DeviceCounter)             # a DeviceCounter that holds nothing: it must not be looked at
    with pytest.raises(ValueError, match="marg_on_device"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=dev, get_marg=False, **kw)
    with pytest.raises(ValueError, match="marg_on_device"):
        get_var_probs.get_bear_probs_seqs(None, ["ACGTA"], 0, counter=dev, get_marg=False, get_map=True, **kw)
