"""ctypes binding of libsequoia_hip.so (the C ABI in include/sequoia_hip.h).

PyTorch is imported first on purpose: the library's NEEDED ``libamdhip64.so.7`` then
resolves to the HIP runtime PyTorch-ROCm already loaded, so device pointers and
streams are shared.  There is no fallback: a missing library or GPU raises.
"""
import ctypes
import os

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
