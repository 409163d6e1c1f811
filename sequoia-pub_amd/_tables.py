"""What the wrappers of the slide analytics (mapstats.py, gtalign.py, spotnorm.py, emd.py) share: a device table, column list or vector
turned into the arguments of the C ABI.  The one way a call is made and a shape is refused is the whole package's: ``_lib.call``."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import call  # noqa: F401  (the analytics wrappers import it from here)


def _on_device(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: a torch tensor on the device is expected, got {type(t).__name__}")
    if not t.is_cuda:
        raise _lib.SequoiaHipError(f"{what}: the tensor is on {t.device}; it must be a CUDA (ROCm) tensor -- there is no CPU fallback")


def table(t, dtypes, what):
    """A device tensor [n, C] whose rows are contiguous -> (tensor, n, C, ld); a column becomes [n, 1]."""
    _on_device(t, what)
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: dtype {t.dtype}, expected one of {[str(d) for d in dtypes]}")
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2:
        raise ValueError(f"{what}: a [n, C] table is expected, got shape {tuple(t.shape)}")
    n, C = t.shape
    if n > 0 and C > 0 and not (t.stride(1) == 1 and (n == 1 or t.stride(0) >= C)):
        t = t.contiguous()
    ld = max(int(t.stride(0)), C, 1) if n > 1 else max(C, 1)
    return t, int(n), int(C), ld


def columns(cols, width, device, what):
    """A column list -> (int32 device tensor or None, count); every index is checked against the table's width first."""
    if cols is None:
        return None, width
    idx = cols.detach().cpu().numpy() if torch.is_tensor(cols) else np.asarray(cols)
    if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
        raise ValueError(f"{what}: cols must be a 1-D list of integer column indices")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= width):
        bad = int(idx[(idx < 0) | (idx >= width)][0])
        raise ValueError(f"{what}: column index {bad} is outside the table's {width} columns")
    return torch.as_tensor(idx.astype(np.int32)).to(device), int(idx.size)


def vector(t, dtype, what):
    """A device vector [n] of the given dtype, contiguous; integer and float inputs are converted."""
    _on_device(t, what)
    if t.dim() != 1:
        raise ValueError(f"{what}: a vector is expected, got shape {tuple(t.shape)}")
    return t.to(dtype).contiguous()


def kept_rows(pred, coords, what):
    """``dropna(how='any')`` over the prediction table and its (name, per-row coordinate vector or None) pairs -> the kept
    rows' numbers on the device and name -> coordinate tensor on the device, the None ones left out."""
    n = int(pred.shape[0])
    keep = ~torch.isnan(pred).any(dim=1)
    named = OrderedDict()
    for name, c in coords:
        if c is None:
            continue
        c = (c if torch.is_tensor(c) else torch.as_tensor(np.array(c))).to(pred.device)
        if c.shape != (n,):
            raise ValueError(f"{what}: {name} has shape {tuple(c.shape)}, expected ({n},)")
        if c.is_floating_point():
            keep &= ~torch.isnan(c)
        named[name] = c
    return torch.nonzero(keep).squeeze(1), named


def empty(dtype, device, *shape):
    """An uninitialised output of the given shape whose pointer is not null even when an extent is 0: a refused shape
    reaches the library, whose message the error then carries."""
    if 0 not in shape:
        return torch.empty(shape, dtype=dtype, device=device)
    return torch.empty([max(s, 1) for s in shape], dtype=dtype, device=device)[tuple(slice(0, s) for s in shape)]
