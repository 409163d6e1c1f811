"""_lib.marshal: what the arguments of ``_lib.call`` become before the stream goes behind them.  Needs the built library and CPU
tensors only; the launch itself is tests/test_gpu_lib_call.py."""
import ctypes

import numpy as np
import pytest
import torch

from sequoia_pub_amd import _lib


def _fn(*args):
    return 0


def test_tensors_slices_and_none():
    flat = torch.arange(16, dtype=torch.float32)
    fn, argv = _lib.marshal(_fn, (flat, flat[5:], None))
    assert fn is _fn
    assert argv[0] == flat.data_ptr() and argv[1] == flat.data_ptr() + 20 and argv[2] is None
    assert _lib.marshal(_fn, (flat[16:],))[1] == [0]                 # the empty tensor is the null pointer, as _lib.ptr sends it


def test_numpy_arrays_go_as_their_data_and_must_be_packed():
    ks = np.asarray([1, 2, 5], dtype=np.int32)
    assert _lib.marshal(_fn, (ks,))[1] == [ks.ctypes.data]
    grid = np.zeros((4, 4), dtype=np.int32)
    assert _lib.marshal(_fn, (grid[1:],))[1] == [grid.ctypes.data + 16]
    for bad in (ks[::2], grid[:, 1], grid.T):
        with pytest.raises(ValueError, match="C-contiguous"):
            _lib.marshal(_fn, (bad,))


def test_everything_else_passes_by_identity():
    cfg = _lib.VisConfig()
    ref, handles, address, scale, count = ctypes.byref(cfg), (ctypes.c_void_p * 2)(), ctypes.c_void_p(64), 0.5, 1 << 40
    argv = _lib.marshal(_fn, (ref, handles, address, scale, count))[1]
    assert all(a is b for a, b in zip(argv, (ref, handles, address, scale, count))) and len(argv) == 5


def test_workspace_pair_comes_last():
    x, ws = torch.zeros(3), torch.empty(48, dtype=torch.uint8)
    assert _lib.marshal(_fn, (x, 7), ws)[1] == [x.data_ptr(), 7, ws.data_ptr(), 48]
    assert _lib.marshal(_fn, (x, 7), None)[1] == [x.data_ptr(), 7]
    assert _lib.marshal(_fn, (x, 7))[1] == [x.data_ptr(), 7]


def test_entry_by_name():
    fn, argv = _lib.marshal("sq_cast_f32_to_bf16", ())
    assert fn is getattr(_lib.lib(), "sq_cast_f32_to_bf16") and argv == []
    with pytest.raises((AttributeError, _lib.SequoiaHipError)):
        _lib.marshal("sq_no_such_entry", (np.zeros(4)[::2],))         # the name is looked up before any argument is


def test_need_returns_the_size_or_raises_the_librarys_sentence():
    L = _lib.lib()
    assert _lib.need(L.sq_slide_mask_workspace_bytes, 64, 64) == L.sq_slide_mask_workspace_bytes(64, 64) > 0
    with pytest.raises(_lib.SequoiaHipArgError) as e:
        _lib.need(L.sq_slide_mask_workspace_bytes, 0, 64)
    assert L.sq_last_error().decode() in str(e.value) and L.sq_last_error()
