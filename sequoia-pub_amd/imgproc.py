"""Image preprocessing on the device.  ``resize_u8_pil``: the resize the reference runs in front of its extractors --
``transforms.Resize(224)`` on a PIL image (/root/reference/pre_processing/compute_features_hdf5.py:53-56,125-126 and
spatial_vis/visualize.py:226-230: ``Image.resize(..., BILINEAR)``) and ``patch.resize(patch_size)``
(pre_processing/patch_gen_hdf5.py:117: BICUBIC) -- for a batch of uint8 patches, bit for bit what Pillow computes
(``sq_resize_u8``, csrc/resize.hip).

The only host arithmetic is Pillow's data-independent coefficient tables (double precision, ``sq_resize_plan_init``),
made and uploaded once per shape."""
import ctypes

import numpy as np
import torch

from . import _abi, _lib

SQ_RESIZE_BILINEAR = _abi.CONSTANTS["SQ_RESIZE_BILINEAR"]
SQ_RESIZE_BICUBIC = _abi.CONSTANTS["SQ_RESIZE_BICUBIC"]
FILTERS = {"bilinear": SQ_RESIZE_BILINEAR, "bicubic": SQ_RESIZE_BICUBIC, SQ_RESIZE_BILINEAR: SQ_RESIZE_BILINEAR,
           SQ_RESIZE_BICUBIC: SQ_RESIZE_BICUBIC}


def resize_plan(h_in, w_in, h_out, w_out, resample="bilinear"):
    """The host plan of sq_resize_plan_init as an int32 array (layout: include/sequoia_hip.h).  Needs no GPU."""
    L = _lib.lib()
    flt = _filter_id(resample)
    need = _lib.need(L.sq_resize_plan_bytes, h_in, w_in, h_out, w_out, flt)
    plan = np.empty(need // 4, dtype=np.int32)
    _lib.check(L.sq_resize_plan_init(h_in, w_in, h_out, w_out, flt, plan.ctypes.data_as(ctypes.c_void_p), need))
    return plan


def _filter_id(resample):
    try:
        return FILTERS[resample]
    except (KeyError, TypeError):
        raise ValueError(f"resample={resample!r}: 'bilinear' or 'bicubic'") from None


_plan_cache = {}


def _device_plan(h_in, w_in, h_out, w_out, flt, dev):
    """The tables depend only on the shapes and the filter: the double arithmetic and the (synchronous, pageable) upload are
    paid once per shape, as kmeans._uniforms does for the seeding draws."""
    key = (int(h_in), int(w_in), int(h_out), int(w_out), int(flt), str(dev))
    hit = _plan_cache.get(key)
    if hit is None:
        plan = resize_plan(h_in, w_in, h_out, w_out, flt)
        if len(_plan_cache) >= 64:
            _plan_cache.clear()
        hit = _plan_cache[key] = torch.from_numpy(plan).to(dev)      # blocking copy: visible to every stream
    return hit


def _gather_args(who, x, index):
    """The checks the gather entries share: ``x`` uint8 [n, H, W, 3 or 4] on the device, ``index`` None or an int32 [m]
    tensor on the same device.  Returns (x contiguous, index contiguous or None, m)."""
    if torch.is_tensor(x) and (x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] not in (3, 4)):      # refused without a GPU too
        raise ValueError(f"{who} takes uint8 [n, H, W, 3 or 4], got {x.dtype} {tuple(x.shape)}")
    _lib.require_gpu()
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.SequoiaHipError(f"{who} needs a CUDA tensor (no CPU fallback)")
    if index is None:
        return x.contiguous(), None, x.shape[0]
    if not (torch.is_tensor(index) and index.is_cuda and index.device == x.device):
        raise _lib.SequoiaHipError(f"{who}: index must be a tensor on the device of the tiles")
    if index.dtype != torch.int32 or index.dim() != 1:
        raise ValueError(f"{who}: index must be int32 [m], got {index.dtype} {tuple(index.shape)}")
    return x.contiguous(), index.contiguous(), index.shape[0]


def resize_u8_pil(patches_u8, size, resample="bilinear", index=None):
    """uint8 [n, H, W, 3] CUDA tensor -> uint8 [n, h, w, 3], every byte equal to
    ``PIL.Image.fromarray(patch).resize((w, h), resample)``.  ``size``: an int (a square output, what ``Resize(224)`` gives a
    square patch) or ``(h, w)``; ``resample``: "bilinear" or "bicubic".  A fourth channel (RGBA as a slide reader returns it)
    is ignored: the result is that of ``patches_u8[..., :3]``.  ``index``: an int32 [m] tensor on the same device; the
    result is then [m, h, w, 3], row j the resize of ``patches_u8[index[j]]`` (``sq_resize_u8_gather``: no gathered copy is
    made); an index outside [0, n) gives a zero image.  Asynchronous on the current stream; no CPU fallback."""
    if index is None and torch.is_tensor(patches_u8) and patches_u8.dim() == 4 and patches_u8.shape[3] == 3:
        return _resize_rgb(patches_u8, size, resample)
    x, idx, m = _gather_args("resize_u8_pil", patches_u8, index)
    h, w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    flt = _filter_id(resample)
    n, H, W, C = x.shape
    dev = x.device
    plan = _device_plan(H, W, h, w, flt, dev)          # refuses a bad size with the library's message before anything is allocated
    out = torch.empty(m, h, w, 3, dtype=torch.uint8, device=dev)
    if m == 0:
        return out
    _lib.call("sq_resize_u8_gather", dev, x, n, C, idx, m, H, W, out, h, w, flt, plan)
    return out


def pack_rgb(tiles_u8, index=None):
    """uint8 [n, H, W, 3 or 4] CUDA tensor -> dense uint8 [m, H, W, 3]: row j is ``tiles_u8[index[j]][..., :3]``
    (``sq_pack_rgb_gather``); ``index`` an int32 [m] tensor on the same device, None for all tiles in order.  An index outside
    [0, n) gives a zero tile.  Asynchronous on the current stream; no CPU fallback."""
    x, idx, m = _gather_args("pack_rgb", tiles_u8, index)
    n, H, W, C = x.shape
    out = torch.empty(m, H, W, 3, dtype=torch.uint8, device=x.device)
    if m == 0:
        return out
    _lib.call("sq_pack_rgb_gather", x.device, x, n, C, idx, m, H, W, out)
    return out


def _resize_rgb(patches_u8, size, resample):
    """resize_u8_pil for three channels and no index: ``sq_resize_u8``."""
    _lib.require_gpu()
    if not (torch.is_tensor(patches_u8) and patches_u8.is_cuda):
        raise _lib.SequoiaHipError("resize_u8_pil needs a CUDA tensor (no CPU fallback)")
    if patches_u8.dtype != torch.uint8 or patches_u8.dim() != 4 or patches_u8.shape[3] != 3:
        raise ValueError(f"resize_u8_pil takes uint8 [n, H, W, 3], got {patches_u8.dtype} {tuple(patches_u8.shape)}")
    h, w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    flt = _filter_id(resample)
    x = patches_u8.contiguous()
    n, H, W, _ = x.shape
    dev = x.device
    plan = _device_plan(H, W, h, w, flt, dev)          # refuses a bad size with the library's message before anything is allocated
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    _lib.call("sq_resize_u8", dev, x, n, H, W, out, h, w, flt, plan)
    return out
