"""Earth mover's distance between a predicted map and its ground truth -- the number the reference's
spatial_vis/get_emd.py exists for (``calculate_emd`` :67-90 and the grid fill and shift of :180-188) -- on the device
(csrc/emd.hip; include/sequoia_hip.h, "Earth mover's distance").

The contract is the OPTIMUM OF THE LINEAR PROGRAM in f64, proven by a certificate: where the reference calls ``cv2.EMD``,
the balanced transportation problem between the two normalised maps is solved exactly (successive shortest augmenting
paths, one workgroup per problem, all problems of a call side by side), and ``return_plan=True`` hands out the feasible
flow and the feasible duals whose equal objectives prove the value without trusting any solver.  ``cv2.EMD`` casts its
signatures to float32 and stops at its own epsilon: it approximates this number and does not define it; no comparison with
cv2 is claimed.  Work is bounded: a cap on augmentations (256 (n + m) by default) and on the flow's arcs; reaching one
raises ``RuntimeError`` naming the problem.  Maps of more than ``MAX_CELLS`` cells of positive weight are refused.  Tensors
live on the device and there is no CPU fallback."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._abi import CONSTANTS as _C
from ._tables import call as _call, columns as _columns, table as _table

MAX_CELLS = _C["SQ_EMD_MAX_CELLS"]                          # cells of positive weight per map
MAX_DIM = _C["SQ_EMD_MAX_DIM"]
MAX_GRID_CELLS = _C["SQ_EMD_MAX_GRID_CELLS"]
MAX_PROBLEMS = _C["SQ_EMD_MAX_PROBLEMS"]
MAX_ARCS = _C["SQ_EMD_MAX_ARCS"]
DEFAULT_AUGMENTATIONS = _C["SQ_EMD_DEFAULT_AUGMENTATIONS"]  # the default cap on augmentations, x (n + m)


def column_chunk():
    """Sink cells one pass of the solver's workgroup covers (``sq_emd_column_chunk``)."""
    return int(_lib.lib().sq_emd_column_chunk())


def _max_augmentations(max_augmentations):
    if max_augmentations is None:
        return 0
    if not isinstance(max_augmentations, (int, np.integer)) or isinstance(max_augmentations, bool) or not 1 <= int(max_augmentations) < 2 ** 31:
        raise ValueError(f"emd: max_augmentations = {max_augmentations!r}, must be None ({DEFAULT_AUGMENTATIONS} (n + m)) or a positive integer")
    return int(max_augmentations)


def _grid_limits(what, P, H, W):
    if P < 1 or P > MAX_PROBLEMS:
        raise ValueError(f"{what}: {P} problems, must be in 1..{MAX_PROBLEMS}")
    if H < 1 or W < 1 or H > MAX_DIM or W > MAX_DIM or H * W > MAX_GRID_CELLS:
        raise ValueError(f"{what}: grid {H} x {W}, both extents must be in 1..{MAX_DIM} and their product at most {MAX_GRID_CELLS}")


def _solve(what, grids, dims, max_aug, return_plan):
    """grids f64 [P, 2, cells] (non-negative, finite), dims int32 [P, 2] on the device -> values f64 [P] (and the plans)."""
    P, cells = int(grids.shape[0]), int(grids.shape[2])
    positive = (grids > 0).sum(dim=2)
    most = int(positive.max())
    if most > MAX_CELLS:
        p = int(torch.nonzero(positive.max(dim=1).values > MAX_CELLS)[0])
        raise ValueError(f"{what}: problem {p} has a map of {int(positive[p].max())} cells with weight; above the limit of {MAX_CELLS} "
                         "(DESIGN.md section 7: out of scope)")
    cap = max(most, 1)
    arc_cap = min(MAX_ARCS, 4 * cap + 128)
    dev = grids.device
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)        # noqa: E731
    value, status, counts = f64(P), i32(P), i32(P, 8)
    cell_a, w_a, cell_b, w_b, u, v = i32(P, cap), f64(P, cap), i32(P, cap), f64(P, cap), f64(P, cap), f64(P, cap)
    arc_i, arc_j, arc_f = i32(P, arc_cap), i32(P, arc_cap), f64(P, arc_cap)
    L = _lib.lib()
    _call(L.sq_emd_solve, dev, grids, cells, dims, P, cap, arc_cap, max_aug, value, status, counts, cell_a, w_a, cell_b, w_b, u, v,
          arc_i, arc_j, arc_f, workspace=int(L.sq_emd_workspace_bytes(P, cap, arc_cap)))
    host = np.ascontiguousarray(status.cpu().numpy())
    try:
        _lib.check(L.sq_emd_status_check(host.ctypes.data_as(ctypes.c_void_p), P))
    except _lib.SequoiaHipError as e:
        raise RuntimeError(f"{what}: {e} (max_augmentations raises the cap on augmentations)") from None
    if not return_plan:
        return value
    cnt, widths = counts.cpu().numpy(), dims[:, 1].cpu().numpy()
    plans = []
    for p in range(P):
        na, nb, W = int(cnt[p, 0]), int(cnt[p, 1]), max(int(widths[p]), 1)
        if na == 0 or nb == 0:                              # a map that is all zero: nothing was solved
            na = nb = 0
        live = torch.nonzero(arc_f[p] > 0).squeeze(1) if na else torch.zeros(0, dtype=torch.int64, device=dev)
        ca, cb = cell_a[p, :na].to(torch.int64), cell_b[p, :nb].to(torch.int64)
        plans.append({"coords_a": torch.stack([ca // W, ca % W], dim=1), "w_a": w_a[p, :na], "coords_b": torch.stack([cb // W, cb % W], dim=1),
                      "w_b": w_b[p, :nb], "u": u[p, :na], "v": v[p, :nb],
                      "arcs": (torch.stack([arc_i[p, live], arc_j[p, live]], dim=1).to(torch.int64), arc_f[p, live]),
                      "augmentations": int(cnt[p, 2]), "steps": int(cnt[p, 4])})
    return value, plans


def emd_grids(arr0, arr1, norm=False, return_plan=False, max_augmentations=None):
    """``calculate_emd(arr0, arr1, norm)`` of get_emd.py:67-90 for a batch of dense f64 device grids [P, H, W] (or [H, W]).
    Returns f64 [P] on the device: 0.0 where both grids are all zero, NaN where exactly one is, otherwise the optimum of
    the transportation problem between the grids divided by their sums (cells of zero weight take no part), with
    sqrt(dx^2 + dy^2) of the cell indices as ground distance.  norm: divided by sqrt(H * H) -- the reference's own
    ``arr1.shape[0] * arr2.shape[0]``, literally.  A negative, NaN or infinite entry raises ValueError.
    return_plan: also a list with, per problem, the kept cells' ``coords_a``, ``coords_b`` (int64 [n, 2]) and weights
    ``w_a``, ``w_b``, the duals ``u``, ``v`` and ``arcs`` = (int64 [k, 2] of (i, j), f64 [k] of flow): the certificate; and the work done,
    ``augmentations`` and search ``steps``.
    max_augmentations: the cap on augmenting paths per problem (None: 256 (n + m), ``DEFAULT_AUGMENTATIONS``); reaching it raises RuntimeError."""
    max_aug = _max_augmentations(max_augmentations)
    if not (torch.is_tensor(arr0) and torch.is_tensor(arr1)):
        raise TypeError("emd_grids: torch tensors on the device are expected")
    if arr0.shape != arr1.shape or arr0.dim() not in (2, 3):
        raise ValueError(f"emd_grids: shapes {tuple(arr0.shape)} and {tuple(arr1.shape)}; two grids [P, H, W] (or [H, W]) of one shape are expected")
    if arr0.dtype != torch.float64 or arr1.dtype != torch.float64:
        raise ValueError(f"emd_grids: dtypes {arr0.dtype} and {arr1.dtype}, expected torch.float64")
    if arr0.dim() == 2:
        arr0, arr1 = arr0.unsqueeze(0), arr1.unsqueeze(0)
    P, H, W = (int(s) for s in arr0.shape)
    _grid_limits("emd_grids", P, H, W)
    _lib.require_gpu()
    if not (arr0.is_cuda and arr1.is_cuda and arr0.device == arr1.device):
        raise _lib.SequoiaHipError(f"emd_grids: the grids are on {arr0.device} and {arr1.device}; both must be on one CUDA (ROCm) device")
    grids = torch.stack([arr0.reshape(P, H * W), arr1.reshape(P, H * W)], dim=1).contiguous()
    if not bool((torch.isfinite(grids) & (grids >= 0)).all()):
        raise ValueError("emd_grids: a grid holds a negative, NaN or infinite entry")
    dims = torch.tensor([[H, W]] * P, dtype=torch.int32, device=grids.device)
    out = _solve("emd_grids", grids, dims, max_aug, return_plan)
    value = out[0] if return_plan else out
    if norm:
        value = value / torch.full_like(value, float(np.sqrt(H * H)))       # tensor / tensor: an IEEE division, no reciprocal
    return (value, out[1]) if return_plan else value


def emd_maps(a, b, xtf, ytf, cols_a=None, cols_b=None, nan_absent=True, norm=False, return_plan=False, max_augmentations=None):
    """The two EMDs of get_emd.py:177-194 for any number of column pairs of one slide at once.  a, b: f64 device tables
    [n, *] over the same n tiles; xtf, ytf: the tiles' non-negative integer grid coordinates.  Problem p compares column
    ``cols_a[p]`` of a with column ``cols_b[p]`` of b (None: every column in order).  Per problem, literally: the grid
    (max x + 1) x (max y + 1) over the rows present, zeros, arr[x, y] = value, arr + abs(min(arr)) with the minimum over the
    whole grid -- with a negative minimum every empty cell becomes positive -- then ``emd_grids``' conventions.
    nan_absent: a row that is NaN in either column is absent from that problem and the grid's extents come from the
    remaining rows (the per-gene dropna of :166); otherwise a NaN raises ValueError.  A problem without any row gives NaN.
    norm: divided by sqrt(H_p * H_p) of the problem's own grid.  Two rows in one grid cell raise ValueError.
    Returns f64 [P] on the device; return_plan as in ``emd_grids``."""
    from .gtalign import _grid_coordinates
    max_aug = _max_augmentations(max_augmentations)
    _lib.require_gpu()
    ta, n, width_a, lda = _table(a, (torch.float64,), "emd_maps: a")
    tb, nb, width_b, ldb = _table(b, (torch.float64,), "emd_maps: b")
    if n != nb or ta.device != tb.device:
        raise ValueError(f"emd_maps: a has {n} rows on {ta.device}, b has {nb} rows on {tb.device}; one set of tiles on one device is expected")
    ca, Pa = _columns(cols_a, width_a, ta.device, "emd_maps: cols_a")
    cb, Pb = _columns(cols_b, width_b, ta.device, "emd_maps: cols_b")
    if Pa != Pb:
        raise ValueError(f"emd_maps: {Pa} columns of a against {Pb} columns of b; one pair per problem is expected")
    P = Pa
    xt, yt, H, W = _grid_coordinates(xtf, ytf, n, ta.device, "emd_maps")
    _grid_limits("emd_maps", P, H, W)
    cells = H * W
    grids = torch.zeros((P, 2, cells), dtype=torch.float64, device=ta.device)
    dims = torch.zeros((P, 2), dtype=torch.int32, device=ta.device)
    flag = torch.zeros(8, dtype=torch.uint8, device=ta.device)
    L = _lib.lib()
    _call(L.sq_emd_fill, ta.device, ta, lda, ca, tb, ldb, cb, n, xt, yt, P, int(bool(nan_absent)), H, W, cells, grids, dims, flag,
          workspace=int(L.sq_emd_fill_workspace_bytes(P, cells)))
    if int(flag[0].item()):
        raise ValueError("emd_maps: two rows share a grid cell (one row per tile is expected)")
    if not bool(torch.isfinite(grids).all()):
        raise ValueError("emd_maps: a map holds a NaN or infinite value" + ("" if nan_absent else " (nan_absent=False: NaN rows are not dropped)"))
    out = _solve("emd_maps", grids, dims, max_aug, return_plan)
    value = out[0] if return_plan else out
    heights = dims[:, 0].to(torch.float64)
    value = torch.where(heights > 0, value, torch.full_like(value, float("nan")))
    if norm:
        value = value / torch.sqrt(heights * heights)
    return (value, out[1]) if return_plan else value
