"""The head and elementwise entry points of the training step (csrc/train.hip), the parts that need
no device: each of eosv_avgpool_forward, eosv_broadcast_rows, eosv_sum_rows, eosv_add_bias,
eosv_nchw_to_nhwc, eosv_flip_weights, eosv_axpy, eosv_sgd_momentum and eosv_softmax_xent, and of the
default conv route eosv_im2col, eosv_col2im, eosv_conv2d_f32 and eosv_conv_wgrad_f32, is exported,
declared in include/eosv.h, and returns EOSV_ERR_ARG with a message naming itself for a null pointer
or a non-positive size, before any device call (the pointers are never dereferenced).  Their
arithmetic is tests/test_gpu_train_kernels.py's and tests/test_gpu_train_convs.py's."""
import ctypes
import os
import re

import pytest

from eosv import _lib

P = 4096  # a non-null address; never dereferenced: every call below fails its argument check

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

# name -> (argument types without the trailing stream, one valid argument list, indices of the
# pointers, indices of the sizes)
ENTRIES = {
    "eosv_avgpool_forward": ([vp, i32, i32, i32, vp], [P, 2, 3, 4, P], [0, 4], [1, 2, 3]),
    "eosv_broadcast_rows": ([vp, i32, i32, i32, f32, vp], [P, 2, 3, 4, 0.5, P], [0, 5], [1, 2, 3]),
    "eosv_sum_rows": ([vp, i32, i32, vp, i32], [P, 2, 3, P, 0], [0, 3], [1, 2]),
    "eosv_add_bias": ([vp, i32, i32, vp], [P, 2, 3, P], [0, 3], [1, 2]),
    "eosv_nchw_to_nhwc": ([vp, i32, i32, i32, i32, vp], [P, 2, 3, 4, 5, P], [0, 5], [1, 2, 3, 4]),
    "eosv_flip_weights": ([vp, i32, i32, i32, i32, vp], [P, 8, 3, 3, 4, P], [0, 5], [1, 2, 3, 4]),
    "eosv_axpy": ([vp, vp, i64, f32], [P, P, 7, 1.0], [0, 1], [2]),
    "eosv_sgd_momentum": ([vp, vp, vp, i64, f32, f32, i32], [P, P, P, 7, 0.1, 0.9, 1], [0, 1, 2], [3]),
    "eosv_softmax_xent": ([vp, vp, i32, i32, vp, vp], [P, P, 2, 5, P, P], [0, 1, 4, 5], [2, 3]),
    # the default conv route (arithmetic: tests/test_gpu_train_convs.py); bias, residual and workspace
    # pointers may be null and are not listed
    "eosv_im2col": ([vp] + [i32] * 8 + [vp], [P, 2, 5, 7, 8, 3, 3, 1, 1, P], [0, 9], [1, 2, 3, 4, 5, 6, 7]),
    "eosv_col2im": ([vp] + [i32] * 8 + [vp], [P, 2, 5, 7, 8, 3, 3, 1, 1, P], [0, 9], [1, 2, 3, 4, 5, 6, 7]),
    "eosv_conv2d_f32": ([vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i64],
                        [P, 2, 5, 7, 32, P, 64, 3, 3, 1, 1, None, None, 0, P, None, 0], [0, 5, 14],
                        [1, 2, 3, 4, 6, 7, 8, 9]),
    "eosv_conv_wgrad_f32": ([vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, i64],
                            [P, 2, 5, 7, 64, P, 64, 3, 3, 1, 1, P, None, 0], [0, 5, 11], [1, 2, 3, 4, 6, 7, 8, 9]),
}


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.eosv_last_error.restype = ctypes.c_char_p
    return L


def _fn(L, name):
    fn = getattr(L, name)
    fn.restype = i32
    fn.argtypes = ENTRIES[name][0] + [vp]
    return fn


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_point_is_exported_and_declared(name):
    L = _library()
    assert hasattr(L, name), name
    assert name in _lib.EXPORTS, name
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eosv.h")
    with open(header) as fh:
        text = fh.read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/eosv.h"


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_pointers_are_rejected_before_any_device_call(name):
    L = _library()
    fn = _fn(L, name)
    _, valid, pointers, _ = ENTRIES[name]
    for i in pointers:
        args = list(valid)
        args[i] = None
        assert fn(*args, None) == -1, (name, i)  # EOSV_ERR_ARG
        assert name.encode() in L.eosv_last_error(), (name, i)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_non_positive_sizes_are_rejected_before_any_device_call(name):
    L = _library()
    fn = _fn(L, name)
    _, valid, _, sizes = ENTRIES[name]
    for i in sizes:
        for bad in (0, -1):
            args = list(valid)
            args[i] = bad
            assert fn(*args, None) == -1, (name, i, bad)
            assert name.encode() in L.eosv_last_error(), (name, i, bad)
