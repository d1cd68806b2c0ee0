"""The convolutional AR function at the protein alphabet's width, the parts that need no GPU: which shapes take the HIP rows
(kernels.cnn_supported), the length of the flat parameter vector against make_ar_func_cnn's own tensors, and the codes
bear_cnn_param_count_wide refuses a shape with."""
import pytest

from bear_amd import _lib, ar_funcs, kernels

MAX_LAG = kernels.CNN_WIDE_MAX_LAG


def test_supported_shapes():
    ok = kernels.cnn_supported
    assert MAX_LAG == 16
    assert ok(1, 20, 1, 30, 16) and ok(12, 20, 8, 30, 16) and ok(16, 20, 16, 30, 16) and ok(16, 20, 1, 30, 16)
    assert not ok(17, 20, 8, 30, 16)            # beyond CNN_WIDE_MAX_LAG
    assert not ok(5, 20, 6, 30, 16)             # filter wider than the context
    assert not ok(5, 20, 0, 30, 16)
    assert not ok(12, 20, 8, 20, 16)            # 20 filters
    assert not ok(12, 20, 8, 30, 8)
    assert not ok(12, 21, 8, 30, 16)
    # the 4-letter alphabets answer as before
    assert ok(13, 4, 8, 30, 16) and ok(21, 4, 21, 30, 16) and ok(17, 4, 8, 30, 16) and ok(1, 4, 1, 30, 16)
    assert not ok(22, 4, 8, 30, 16) and not ok(5, 4, 6, 30, 16) and not ok(13, 4, 8, 20, 16) and not ok(13, 4, 8, 30, 8)


@pytest.mark.parametrize("lag,fw", [(12, 8), (5, 3), (8, 8), (4, 1), (1, 1), (16, 8), (16, 16), (16, 1)])
def test_param_count_matches_the_parameter_tensors(lag, fw):
    f, params = ar_funcs.make_ar_func_cnn(lag, 20, filter_width=fw)
    assert f.fused
    assert kernels.cnn_param_count_wide(lag, fw) == sum(p.numel() for p in params)
    if (lag, fw) == (12, 8):
        assert kernels.cnn_param_count_wide(lag, fw) == 8129


def test_param_count_refusals():
    count = _lib.lib().bear_cnn_param_count_wide
    assert count(12, 8, 30, 16, 21) == 8129
    for args in [(12, 8, 30, 16, 5), (12, 8, 30, 16, 20), (12, 8, 20, 16, 21), (12, 8, 30, 8, 21), (12, 0, 30, 16, 21),
                 (12, 13, 30, 16, 21), (MAX_LAG + 1, 8, 30, 16, 21), (0, 0, 30, 16, 21), (-1, 1, 30, 16, 21)]:
        assert count(*args) == -1, args          # BEAR_ERR_INVALID_ARG
    with pytest.raises(_lib.BearError):
        kernels.cnn_param_count_wide(MAX_LAG + 1, 8)
    assert not ar_funcs.make_ar_func_cnn(MAX_LAG + 1, 20, filter_width=8)[0].fused
    assert not ar_funcs.make_ar_func_cnn(12, 20, filter_width=8, num_filters=20)[0].fused
