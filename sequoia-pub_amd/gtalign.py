"""Alignment of a predicted slide with its spatial-transcriptomics ground truth -- ``get_average``, ``median_filter`` and
the ``np.unique`` counts of the reference's spatial_vis/get_emd.py on the device (csrc/gtalign.hip; include/sequoia_hip.h,
"Ground-truth alignment").

The reference finds the four nearest spots of every tile by sorting ALL spot distances in Python, once per tile and again
for every gene, and filters the result with a pandas scan per row.  The nearest spots do not depend on the gene: here they
are found once (``nearest_spots``) and serve every gene through a gather (``spot_means``); the 3 x 3 median over the
sparse tile grid (``median_filter``) and the distinct-value counts (``count_unique``) take all genes in one call.  Every
result equals the reference's own call bit for bit (NaN signs and payloads aside).  Tensors live on the device and there
is no CPU fallback.  The EMD itself -- the grid fill, the normalisation and the transportation problem the reference hands
to cv2.EMD -- is emd.py (csrc/emd.hip); ``align_ground_truth(..., emd=True)`` adds its two columns.  The figures stay out
(DESIGN.md section 7)."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._abi import CONSTANTS as _C
from ._tables import call as _call, columns as _columns, empty as _empty, kept_rows as _kept_rows, table as _table, vector as _vector
from .mapstats import MAX_ROWS, percentile_of_score

MAX_SPOTS = _C["SQ_GT_MAX_SPOTS"]
MAX_K = _C["SQ_GT_MAX_K"]
MAX_RADIUS = _C["SQ_GT_MAX_RADIUS"]
MAX_GRID_CELLS = _C["SQ_GT_MAX_GRID_CELLS"]
MAX_UNIQUE_COLS = _C["SQ_GT_MAX_UNIQUE_COLS"]


def spot_chunk():
    """Spots of one LDS chunk of the nearest-spot kernel (``sq_gt_spot_chunk``)."""
    return int(_lib.lib().sq_gt_spot_chunk())


def unique_chunk_rows():
    """Rows of one sorted chunk of a column (``sq_gt_unique_chunk_rows``)."""
    return int(_lib.lib().sq_gt_unique_chunk_rows())


def _neighbour_count(num_tiles):
    if not isinstance(num_tiles, (int, np.integer)) or isinstance(num_tiles, bool) or not 1 <= int(num_tiles) <= MAX_K:
        raise ValueError(f"nearest_spots: num_tiles = {num_tiles!r}, must be an integer in 1..{MAX_K}")
    return int(num_tiles)


def nearest_spots(xcoord, ycoord, spot_x, spot_y, num_tiles=4, return_distances=False):
    """``sorted(range(n_spots), key=lambda i: distances[i])[:num_tiles]`` of get_emd.py:29-32 for every tile at once.
    xcoord, ycoord: device vectors [n_tiles]; spot_x, spot_y: device vectors [n_spots] (converted to f64).  Returns int32
    [n_tiles, min(num_tiles, n_spots)]: the nearest spots in the stable sort's order (equal distance: the lower spot
    index); return_distances: also their f64 distances.  A NaN coordinate is refused (Python's ``sorted`` has no defined
    order for it)."""
    k = _neighbour_count(num_tiles)
    if not all(torch.is_tensor(t) for t in (xcoord, ycoord, spot_x, spot_y)):
        raise TypeError("nearest_spots: torch tensors on the device are expected")
    if xcoord.shape != ycoord.shape or spot_x.shape != spot_y.shape:
        raise ValueError(f"nearest_spots: xcoord {tuple(xcoord.shape)} / ycoord {tuple(ycoord.shape)} or spot_x {tuple(spot_x.shape)} / "
                         f"spot_y {tuple(spot_y.shape)} differ in shape")
    _lib.require_gpu()
    xc, yc = _vector(xcoord, torch.float64, "nearest_spots: xcoord"), _vector(ycoord, torch.float64, "nearest_spots: ycoord")
    sx, sy = _vector(spot_x, torch.float64, "nearest_spots: spot_x"), _vector(spot_y, torch.float64, "nearest_spots: spot_y")
    n_tiles, n_spots = int(xc.numel()), int(sx.numel())
    if n_tiles and n_spots and bool(torch.stack([torch.isnan(xc).any(), torch.isnan(yc).any(), torch.isnan(sx).any(), torch.isnan(sy).any()]).any()):
        raise ValueError("nearest_spots: a coordinate is NaN")
    k_eff = max(1, min(k, n_spots))
    idx = _empty(torch.int32, xc.device, n_tiles, k_eff)
    dist = _empty(torch.float64, xc.device, n_tiles, k_eff) if return_distances else None
    _call(_lib.lib().sq_gt_nearest_spots, xc.device, xc, yc, n_tiles, sx, sy, n_spots, k, idx, dist)
    return (idx, dist) if return_distances else idx


def spot_means(idx, expr, cols=None):
    """``np.mean`` of the kept spots' expression (get_emd.py:34-38) for every tile and every column.  idx: int32 device
    tensor [n_tiles, k] from ``nearest_spots``; expr: f32 or f64 device table [n_spots, width]; cols: which columns, in
    which order (None: all).  Returns f64 [n_tiles, C]: numpy's sum of the k values in kept order over k; a NaN or an
    infinity propagates."""
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int32:
        raise ValueError("spot_means: idx must be an int32 tensor [n_tiles, k]")
    _lib.require_gpu()
    t, n_spots, width, ld = _table(expr, (torch.float32, torch.float64), "spot_means")
    if not idx.is_cuda or idx.device != t.device:
        raise _lib.SequoiaHipError(f"spot_means: idx is on {idx.device}, expr on {t.device}; both must be on one CUDA (ROCm) device")
    col_t, C = _columns(cols, width, t.device, "spot_means")
    idx = idx.contiguous()
    n_tiles, k_eff = int(idx.shape[0]), int(idx.shape[1])
    out = _empty(torch.float64, t.device, n_tiles, C)
    _call(_lib.lib().sq_gt_spot_means, t.device, idx, n_tiles, k_eff, t, int(t.dtype == torch.float64), n_spots, ld, col_t, C, out)
    return out


def _grid_coordinates(xtf, ytf, n, device, what):
    """int32 device vectors and the grid extents; one download of the four extrema."""
    out = []
    for name, c in (("xtf", xtf), ("ytf", ytf)):
        c = torch.as_tensor(np.array(c)) if not torch.is_tensor(c) else c
        if c.dim() != 1 or c.numel() != n:
            raise ValueError(f"{what}: {name} has shape {tuple(c.shape)}, expected ({n},)")
        if c.is_floating_point():
            if bool((c != c.round()).any()) or bool(torch.isnan(c).any()):
                raise ValueError(f"{what}: {name} holds a value that is no integer")
        out.append(c.to(device))
    if n == 0:
        return out[0].to(torch.int32), out[1].to(torch.int32), 1, 1
    ext = torch.stack([out[0].min(), out[0].max(), out[1].min(), out[1].max()]).cpu().tolist()
    if ext[0] < 0 or ext[2] < 0:
        raise ValueError(f"{what}: a grid coordinate is negative (xtf from {int(ext[0])}, ytf from {int(ext[2])})")
    if ext[1] >= 2 ** 31 - 1 or ext[3] >= 2 ** 31 - 1:
        raise ValueError(f"{what}: a grid coordinate does not fit 32 bits")
    return out[0].to(torch.int32).contiguous(), out[1].to(torch.int32).contiguous(), int(ext[1]) + 1, int(ext[3]) + 1


def median_filter(values, xtf, ytf, num_neighbors=1, nan_absent=False, cols=None, return_counts=False):
    """``median_filter(df, col, x, y, num_neighbors)`` of get_emd.py:41-51 for every row of every column.  values: f64
    device tensor [n, width] (or [n]); xtf, ytf: the rows' non-negative integer grid coordinates, one row per cell.  A
    row whose (2 r + 1)^2 window holds more than half its cells' worth of rows gets ``np.median`` of the window, any other
    row keeps its own value.  nan_absent: a NaN in column c means the row is absent from column c (the reference's
    per-gene ``dropna``): no window of that column counts it and its own result is NaN; otherwise a NaN member makes the
    median NaN, as ``np.median`` does.  Returns f64 [n, C] ([n] for a vector); return_counts: also the windows' row counts,
    int32 of the same shape.  Two rows in one grid cell raise ValueError."""
    _lib.require_gpu()
    t, n, width, ld = _table(values, (torch.float64,), "median_filter")
    col_t, C = _columns(cols, width, t.device, "median_filter")
    xt, yt, grid_w, grid_h = _grid_coordinates(xtf, ytf, n, t.device, "median_filter")
    r = int(num_neighbors)
    L = _lib.lib()
    out = _empty(torch.float64, t.device, n, C)
    counts = _empty(torch.int32, t.device, n, C) if return_counts else None
    flag = torch.zeros(8, dtype=torch.uint8, device=t.device)
    _call(L.sq_gt_median_filter, t.device, t, n, ld, col_t, C, xt, yt, grid_w, grid_h, r, int(bool(nan_absent)), out, counts, flag,
          workspace=int(L.sq_gt_median_filter_workspace_bytes(n, grid_w, grid_h)))
    if int(flag[0].item()):
        raise ValueError("median_filter: two rows share a grid cell (one row per tile is expected)")
    if torch.is_tensor(values) and values.dim() == 1:
        out = out[:, 0]
        counts = counts[:, 0] if return_counts else None
    return (out, counts) if return_counts else out


def count_unique(values, cols=None):
    """``len(np.unique(column))`` (get_emd.py:204-205) of every column of the f64 device tensor values [n, width] (or [n]):
    int32 [C] on the device.  -0.0 and 0.0 are one value; all NaNs together are one."""
    _lib.require_gpu()
    t, n, width, ld = _table(values, (torch.float64,), "count_unique")
    col_t, C = _columns(cols, width, t.device, "count_unique")
    L = _lib.lib()
    out = _empty(torch.int32, t.device, C)
    _call(L.sq_gt_count_unique, t.device, t, n, ld, col_t, C, out, workspace=int(L.sq_gt_count_unique_workspace_bytes(n, C)))
    return out


def _gene_columns(gene_names, genes):
    where = {}
    for i, g in enumerate(gene_names):
        where.setdefault(g, i)
    missing = [g for g in genes if g not in where]
    if missing:
        raise ValueError(f"align_ground_truth: genes {missing[:5]} are no columns of the prediction table")
    return [where[g] for g in genes]


def align_ground_truth(pred, gene_names, xcoord, ycoord, xtf, ytf, spot_x, spot_y, spot_expr, genes, num_tiles=4, emd=False, max_augmentations=None):
    """get_emd.py:163-175 and :204-205 for all requested genes of one slide at once.

    pred: f32 device tensor [n_tiles, G] whose columns are ``gene_names``; xcoord, ycoord: the tiles' pixel coordinates and
    xtf, ytf their grid coordinates (the columns of stride-1.csv); spot_x, spot_y: the spots' coordinates; spot_expr: f32 or
    f64 device table [n_spots, len(genes)], column j holding the (already normalised) expression of ``genes[j]``.

    Rows with any NaN are dropped (:164).  The ``num_tiles`` nearest spots of every tile are found ONCE; per gene the
    ground truth is their mean expression (:165), rows where it is NaN leave that gene (:166), the rest is median-filtered
    over the tile grid and turned into its percentile within the slide (:170-172), and so is the prediction (:174-175).
    Returns two DataFrames: per tile, indexed by the kept rows' positions, xcoord, ycoord, xcoord_tf, ycoord_tf and per
    gene ``<gene>`` (the prediction), ``<gene>_ground_truth``, ``<gene>_ground_truth_filt`` (the percentile of the filtered
    ground truth) and ``<gene>_filt`` (the percentile of the prediction), NaN where the gene's ground truth is NaN; and
    per gene ``gene, nr_gt_vals, nr_gt_vals_filt``: the distinct values of the two ground-truth columns.

    emd=True: the second frame carries the reference's columns in its merge order (:213-222), ``gene, emd, nr_gt_vals,
    emd_filt, nr_gt_vals_filt``: ``emd`` is the earth mover's distance (emd.emd_maps: :177-194) between the prediction and
    ``ground_truth`` over the gene's rows, ``emd_filt`` between ``<gene>_filt`` and ``ground_truth_filt``; all genes and
    both variants are solved in one batched call; max_augmentations is emd_maps' cap on the augmenting paths of one problem
    (None: its default).  Without emd every output is what it was."""
    import pandas as pd
    k = _neighbour_count(num_tiles)
    genes = list(genes)
    if not genes:
        raise ValueError("align_ground_truth: no genes requested")
    if not torch.is_tensor(pred) or pred.dim() != 2 or pred.shape[1] != len(gene_names):
        raise ValueError(f"align_ground_truth: pred does not have one column per gene name ({len(gene_names)})")
    gene_cols = _gene_columns(gene_names, genes)
    if not torch.is_tensor(spot_expr) or spot_expr.dim() != 2 or spot_expr.shape[1] != len(genes):
        raise ValueError(f"align_ground_truth: spot_expr does not have one column per requested gene ({len(genes)})")
    rows, named = _kept_rows(pred, (("xcoord", xcoord), ("ycoord", ycoord), ("xcoord_tf", xtf), ("ycoord_tf", ytf)), "align_ground_truth")
    n, m = int(pred.shape[0]), int(rows.numel())
    frame = OrderedDict((name, c[rows].cpu().numpy()) for name, c in named.items())
    if m == 0:
        for g in genes:
            for col in (g, g + "_ground_truth", g + "_ground_truth_filt", g + "_filt"):
                frame[col] = np.zeros(0)
        counts = pd.DataFrame({"gene": genes, "nr_gt_vals": [0] * len(genes), "nr_gt_vals_filt": [0] * len(genes)})
        if emd:
            counts.insert(1, "emd", np.nan)
            counts.insert(3, "emd_filt", np.nan)
        return pd.DataFrame(frame, index=rows.cpu().numpy()), counts
    kept = pred if m == n else pred[rows]
    idx = nearest_spots(named["xcoord"][rows], named["ycoord"][rows], spot_x, spot_y, num_tiles=k)
    gt = spot_means(idx, spot_expr)
    filt = median_filter(gt, named["xcoord_tf"][rows], named["ycoord_tf"][rows], num_neighbors=1, nan_absent=True)
    has_nan = torch.isnan(gt).any(dim=0).cpu().numpy()
    clean = [j for j in range(len(genes)) if not has_nan[j]]
    nan = float("nan")
    perc_gt = torch.full((m, len(genes)), nan, dtype=torch.float64, device=pred.device)
    perc_pred = torch.full((m, len(genes)), nan, dtype=torch.float64, device=pred.device)
    nr_gt = np.zeros(len(genes), dtype=np.int64)
    nr_filt = np.zeros(len(genes), dtype=np.int64)
    if clean:                                               # every gene without a NaN: one call each for all of them
        perc_gt[:, clean] = percentile_of_score(filt, cols=clean)
        perc_pred[:, clean] = percentile_of_score(kept, cols=[gene_cols[j] for j in clean])
        nr_gt[clean] = count_unique(gt, cols=clean).cpu().numpy()
        nr_filt[clean] = count_unique(perc_gt, cols=clean).cpu().numpy()
    for j in range(len(genes)):                             # a gene's own dropna (:166): its rows compacted
        if not has_nan[j]:
            continue
        sub = torch.nonzero(~torch.isnan(gt[:, j])).squeeze(1)
        if sub.numel() == 0:
            continue
        pg = percentile_of_score(filt[sub, j].contiguous())
        perc_gt[sub, j] = pg[:, 0]
        perc_pred[sub, j] = percentile_of_score(kept[sub, gene_cols[j]].contiguous())[:, 0]
        nr_gt[j] = int(count_unique(gt[sub, j].contiguous())[0])
        nr_filt[j] = int(count_unique(pg)[0])
    absent = torch.isnan(gt)
    pred_cols = kept[:, gene_cols].to(torch.float64)
    pred_cols[absent] = nan
    gt_h, pg_h, pp_h, pr_h = gt.cpu().numpy(), perc_gt.cpu().numpy(), perc_pred.cpu().numpy(), pred_cols.cpu().numpy()
    for j, g in enumerate(genes):
        frame[g] = pr_h[:, j]
        frame[g + "_ground_truth"] = gt_h[:, j]
        frame[g + "_ground_truth_filt"] = pg_h[:, j]
        frame[g + "_filt"] = pp_h[:, j]
    counts = pd.DataFrame({"gene": genes, "nr_gt_vals": nr_gt, "nr_gt_vals_filt": nr_filt})
    if emd:                                                 # raw and percentile maps of every gene: 2 G problems, one call
        from .emd import emd_maps
        G = len(genes)
        dist = emd_maps(torch.cat([pred_cols, perc_pred], dim=1), torch.cat([gt, perc_gt], dim=1), named["xcoord_tf"][rows],
                        named["ycoord_tf"][rows], nan_absent=True, max_augmentations=max_augmentations).cpu().numpy()
        counts.insert(1, "emd", dist[:G])
        counts.insert(3, "emd_filt", dist[G:])
    return pd.DataFrame(frame, index=rows.cpu().numpy()), counts
