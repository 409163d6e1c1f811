"""ctypes binding of libsequoia_hip.so (the C ABI in include/sequoia_hip.h).

PyTorch is imported first on purpose: the library's NEEDED ``libamdhip64.so.7`` then
resolves to the HIP runtime PyTorch-ROCm already loaded, so device pointers and
streams are shared.  There is no fallback: a missing library or GPU raises.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede CDLL, see module docstring)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SQ_HIP_LIB") or os.path.join(_HERE, "libsequoia_hip.so")      # SQ_HIP_LIB: another build of the library (same-box A/B runs)

_C = _abi.CONSTANTS
SQ_F32, SQ_BF16 = _C["SQ_DTYPE_F32"], _C["SQ_DTYPE_BF16"]
SQ_BF16X3 = _C["SQ_DTYPE_BF16X3"]       # split bf16 (hi + lo planes, three MFMAs per product): ResNet-50 embedder only
SQ_F16X3 = _C["SQ_DTYPE_F16X3"]         # the same with fp16 planes (22 significant bits, range 65504): the fast parity mode
SQ_MAX_DEPTH, HEAD_DIM = _C["SQ_MAX_DEPTH"], _C["SQ_HEAD_DIM"]
SQ_OK, SQ_ERR_ARG = _C["SQ_OK"], _C["SQ_ERR_ARG"]

DTYPES = {"fp32": SQ_F32, "f32": SQ_F32, "float32": SQ_F32, SQ_F32: SQ_F32,
          "bf16": SQ_BF16, "bfloat16": SQ_BF16, SQ_BF16: SQ_BF16,
          "bf16x3": SQ_BF16X3, "split-bf16": SQ_BF16X3, SQ_BF16X3: SQ_BF16X3,
          "f16x3": SQ_F16X3, "fp16x3": SQ_F16X3, "split-fp16": SQ_F16X3, SQ_F16X3: SQ_F16X3}

VisConfig, VisLayerOffsets, VisLayout = (_abi.STRUCTS[n] for n in ("sq_vis_config", "sq_vis_layer_offsets", "sq_vis_layout"))
VitConfig, VitLayerOffsets, VitLayout = (_abi.STRUCTS[n] for n in ("sq_vit_config", "sq_vit_layer_offsets", "sq_vit_layout"))
ConvDesc, ResNet50Layout = _abi.STRUCTS["sq_conv_desc"], _abi.STRUCTS["sq_resnet50_layout"]


class SequoiaHipError(RuntimeError):
    pass


class SequoiaHipArgError(SequoiaHipError, ValueError):
    """The library refused an argument (SQ_ERR_ARG)."""


_lib = None


def _declare(lib):
    """restype and argtypes of every function the header declares; a declared symbol the library lacks is an error."""
    for name, (restype, argtypes) in _abi.FUNCTIONS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise SequoiaHipError(f"{LIB_PATH} does not export {name}, which include/sequoia_hip.h declares: rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes


def lib():
    """Load (once) and return the shared library; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SequoiaHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or sequoia-pub_amd/csrc/build.sh).  sequoia-pub_amd has no CPU fallback.")
        loaded = ctypes.CDLL(LIB_PATH)
        _declare(loaded)
        _lib = loaded
    return _lib


def check(rc):
    if rc != SQ_OK:
        kind = SequoiaHipArgError if rc == SQ_ERR_ARG else SequoiaHipError
        raise kind(f"libsequoia_hip error {rc}: {lib().sq_last_error().decode()}")


def require_gpu(device=None):
    """The product path runs on MI355X only: fail loudly otherwise."""
    if not torch.cuda.is_available():
        raise SequoiaHipError("no ROCm GPU visible to PyTorch: the HIP path cannot run (and there is no CPU fallback)")
    if not lib().sq_device_ok():
        raise SequoiaHipError("the visible GPU is not gfx950 (MI355X); libsequoia_hip is built for gfx950 only")


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def need(fn, *args):
    """The byte count an entry's ``*_workspace_bytes`` (or ``*_bytes``) function asks for.  It is 0 exactly for the shapes the entry
    refuses (include/sequoia_hip.h): that raises the library's own sentence (sq_last_error) as a ``SequoiaHipArgError``."""
    n = fn(*args)
    if n == 0:
        check(SQ_ERR_ARG)
    return n


def marshal(fn, args, workspace=None):
    """(fn, args) of ``call`` as ctypes takes them, the stream left out; touches no device.  ``fn``: a ctypes function or an
    entry's name.  A tensor goes as its address (a slice as the address of its first element, an empty one as 0), a numpy
    array -- C-contiguous, or ValueError -- as the address of its data; None (the null pointer), numbers, ``ctypes.byref``, ctypes
    arrays and ``c_void_p`` pass as they are.  ``workspace``: a uint8 tensor whose address and size in bytes come last."""
    if isinstance(fn, str):
        fn = getattr(lib(), fn)
    out = []
    for a in args:
        if isinstance(a, torch.Tensor):
            a = a.data_ptr()
        elif isinstance(a, np.ndarray):
            if not a.flags.c_contiguous:
                raise ValueError(f"{fn.__name__}: a numpy argument of shape {a.shape} is not C-contiguous; the library reads packed arrays")
            a = a.ctypes.data
        out.append(a)
    if workspace is not None:
        out += [workspace.data_ptr(), workspace.numel()]
    return fn, out


def call(fn, device, *args, workspace=None, after=()):
    """One library launch on ``device`` and its current stream: the arguments as ``marshal`` turns them, then the workspace pair, then
    the stream, read under the device guard at call time (so a call inside ``torch.cuda.stream(s)`` lands on ``s``), then ``after`` as
    it is (sq_vis_backward_buckets takes its events behind the stream).  The library keys per-device state (its once-flags, side
    streams and profiler slots) on the current device: the guard is here so that no launch can be made without it.
    workspace: a uint8 tensor the caller keeps, or a byte count -- the entry's ``*_workspace_bytes`` -- for scratch of that size.
    The count is 0 exactly for the shapes the entry refuses, so nothing is tested here: the one real call is made, the library's
    own first check refuses it and ``check`` raises its message (a ``SequoiaHipArgError``).
    ``args`` holds every tensor and array, temporaries made in the argument list too, until the entry has returned."""
    if workspace is not None and not isinstance(workspace, torch.Tensor):
        args += (torch.empty(max(workspace, 8), dtype=torch.uint8, device=device), workspace)
        workspace = None
    fn, argv = marshal(fn, args, workspace)
    with torch.cuda.device(device):
        check(fn(*argv, stream_ptr(device), *after))


def prof_enable(on, markers=False):
    """HIP-event timing of the library's launches on / off; markers=True: sq_prof_enable(2), marker launches around every one."""
    check(lib().sq_prof_enable(2 if (on and markers) else int(bool(on))))


def prof_marker_names():
    import json
    buf = ctypes.create_string_buffer(1 << 18)
    check(lib().sq_prof_marker_names(buf, len(buf)))
    return json.loads(buf.value.decode())


def prof_report():
    """Per-kernel HIP-event timings recorded since prof_enable(True) (synchronises first)."""
    import json
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 20)
    check(lib().sq_prof_report(buf, len(buf)))
    return json.loads(buf.value.decode())
