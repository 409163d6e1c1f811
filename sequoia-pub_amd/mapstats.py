"""Cell-type maps and gene co-expression of a predicted slide -- the numeric part of
/root/reference/spatial_vis/gbm_celltype_analysis.py and the percentile step of spatial_vis/get_emd.py, on the device
(csrc/mapstats.hip; include/sequoia_hip.h, "Map statistics").

The table these scripts read is the f32 ``[n_tiles, G]`` prediction table ``spatial.sliding_window_all_genes`` leaves on
the device.  The reference ranks every tile with one ``scipy.stats.percentileofscore`` call per row (O(n) each) and
correlates the genes with ``DataFrame.corr()`` on one core; here both are one library call.  Tensors live on the device
and there is no CPU fallback.  The alignment with the spatial-transcriptomics ground truth is gtalign.py; figures and the EMD stay out
(DESIGN.md section 7)."""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._abi import CONSTANTS as _C
from ._tables import call as _call, columns as _columns, empty as _empty, kept_rows as _kept_rows, table as _table

MAX_ROWS = _C["SQ_MAP_MAX_ROWS"]
MAX_CORR_COLS = _C["SQ_MAP_MAX_CORR_COLS"]
LABELS = ("ac", "cc", "mes", "lin")
# gbm_celltype_analysis.py:44-47,102 (the reference's names: 'purple' is the teal, 'green' the ochre)
COLORS = OrderedDict([("ac", "#36CEBC"), ("cc", "#CE3649"), ("mes", "#3648CE"), ("lin", "#CEBC36")])


def rank_chunk_rows():
    """Rows of one sorted chunk of a column (``sq_map_rank_chunk_rows``)."""
    return int(_lib.lib().sq_map_rank_chunk_rows())


def percentile_of_score(values, cols=None, return_argmax=False):
    """``scipy.stats.percentileofscore(column, x)`` (kind='rank') for every element x of every column, bit-equal to scipy
    (gbm_celltype_analysis.py:12-16,107; get_emd.py:21-25,172,175).  values: f32 or f64 device tensor [n, width] (or [n]);
    cols: which columns, in which order (None: all).  Returns f64 [n, C]; a column holding a NaN comes back all NaN.
    return_argmax: also int32 [n], the first column with the row's largest percentile (NaN skipped, -1 for a row of NaN):
    ``idxmax(axis=1)`` of :109."""
    _lib.require_gpu()
    t, n, width, ld = _table(values, (torch.float32, torch.float64), "percentile_of_score")
    col_t, C = _columns(cols, width, t.device, "percentile_of_score")
    f64 = int(t.dtype == torch.float64)
    L = _lib.lib()
    out = _empty(torch.float64, t.device, n, C)
    arg = _empty(torch.int32, t.device, n) if return_argmax else None
    scale = 50.0 / n if n else 0.0                          # no rows: the call is refused whatever the scale
    _call(L.sq_map_percentile, t.device, t, f64, n, ld, col_t, C, scale, out, arg, workspace=int(L.sq_map_percentile_workspace_bytes(n, C, f64)))
    return (out, arg) if return_argmax else out


def _category_lists(categories, width):
    lists = list(categories.values()) if hasattr(categories, "values") else list(categories)
    lists = [np.asarray(list(c), dtype=np.int64).reshape(-1) for c in lists]
    for k, c in enumerate(lists):
        if c.size and (int(c.min()) < 0 or int(c.max()) >= width):
            bad = int(c[(c < 0) | (c >= width)][0])
            raise ValueError(f"category_means: gene index {bad} of category {k} is outside the table's {width} columns")
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([c.size for c in lists])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("category_means: more than 2^31 - 1 category members")
    members = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
    return members.astype(np.int32), offsets.astype(np.int32)


def category_means(pred, categories):
    """``df[genes of the category].mean(axis=1)`` (gbm_celltype_analysis.py:105) for every category at once.  pred: f32
    device tensor [n, G]; categories: a sequence (or ordered mapping) of lists of gene COLUMN indices, duplicates kept.
    Every index is checked against G before anything is uploaded.  Returns f64 [n, n_cat]: the f64 sum of the members in
    list order over their count; NaN for an empty category, as pandas."""
    _lib.require_gpu()
    t, n, width, ld = _table(pred, (torch.float32,), "category_means")
    members, offsets = _category_lists(categories, width)
    n_cat = len(offsets) - 1
    mem_t = torch.as_tensor(members).to(t.device) if members.size else None
    off_t = torch.as_tensor(offsets).to(t.device)
    out = _empty(torch.float64, t.device, n, n_cat)
    _call(_lib.lib().sq_map_category_means, t.device, t, n, ld, mem_t, int(members.size), off_t, n_cat, out)
    return out


def gene_correlation(pred, cols=None):
    """``df[genes].corr()`` (Pearson; gbm_celltype_analysis.py:75) of K columns of the f32 device table pred [n, G]:
    f64 [K, K], bit-symmetric, diagonal exactly 1.0, NaN in the row and column of a constant gene (as pandas)."""
    _lib.require_gpu()
    t, n, width, ld = _table(pred, (torch.float32,), "gene_correlation")
    col_t, K = _columns(cols, width, t.device, "gene_correlation")
    L = _lib.lib()
    need = int(L.sq_map_gene_corr_workspace_bytes(n, K))
    out = _empty(torch.float64, t.device, *((K, K) if need else (1, 1)))      # a refused K may be too many columns to square
    _call(L.sq_map_gene_corr, t.device, t, n, ld, col_t, K, out, workspace=need)
    return out


def category_indices(gene_names, categories):
    """label -> column indices of the category's genes in ``gene_names``; names that are absent are skipped, as
    ``[i for i in categories[j] if i in df.columns]`` does (:105), duplicates and list order kept."""
    where = {}
    for i, g in enumerate(gene_names):
        where.setdefault(g, i)
    return OrderedDict((label, [where[g] for g in names if g in where]) for label, names in categories.items())


def celltype_maps(pred, gene_names, categories, xtf=None, ytf=None, colors=None):
    """gbm_celltype_analysis.py:97-111 for one slide.  pred: f32 device tensor [n_tiles, G] whose columns are
    ``gene_names``; categories: ordered mapping label -> gene names; xtf / ytf: the tiles' grid coordinates (optional).
    Rows holding any NaN are dropped (``dropna(how='any')``), then per label the mean over the category's genes and its
    percentile within the slide, then ``color``: the colour of the label with the first largest percentile.  Returns a
    DataFrame indexed by the kept rows' positions with the columns [xcoord_tf, ycoord_tf,] <label>, <label>_perc, ...,
    color."""
    import pandas as pd
    colors = COLORS if colors is None else colors
    labels = list(categories.keys())
    index_lists = category_indices(gene_names, categories)
    if pred.dim() != 2 or pred.shape[1] != len(gene_names):
        raise ValueError(f"celltype_maps: pred {tuple(pred.shape)} does not have one column per gene name ({len(gene_names)})")
    rows, coords = _kept_rows(pred, (("xcoord_tf", xtf), ("ycoord_tf", ytf)), "celltype_maps")
    frame = OrderedDict((name, c[rows].cpu().numpy()) for name, c in coords.items())
    if rows.numel() == 0:
        for label in labels:
            frame[label] = np.zeros(0)
            frame[label + "_perc"] = np.zeros(0)
        frame["color"] = np.zeros(0, dtype=object)
        return pd.DataFrame(frame, index=rows.cpu().numpy())
    kept = pred if rows.numel() == pred.shape[0] else pred[rows]
    means = category_means(kept, index_lists)
    perc, first = percentile_of_score(means, return_argmax=True)
    means, perc, first = means.cpu().numpy(), perc.cpu().numpy(), first.cpu().numpy()
    for k, label in enumerate(labels):
        frame[label] = means[:, k]
        frame[label + "_perc"] = perc[:, k]
    palette = np.array([colors[label] for label in labels] + [np.nan], dtype=object)
    frame["color"] = palette[first]                        # -1 (a row of NaN percentiles) -> NaN, as idxmax + map give
    return pd.DataFrame(frame, index=rows.cpu().numpy())


def mean_correlation(frames):
    """gbm_celltype_analysis.py:137-140: the label-aligned sum of the per-slide correlation frames over their number."""
    frames = list(frames)
    if not frames:
        raise ValueError("mean_correlation: no correlation frames")
    total = frames[0]
    for f in frames[1:]:
        total = total + f
    return total / len(frames)
