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
from ._tables import _on_device, call as _call, columns as _columns, empty as _empty, kept_rows as _kept_rows, table as _table

MAX_ROWS = _C["SQ_MAP_MAX_ROWS"]
MAX_CORR_COLS = _C["SQ_MAP_MAX_CORR_COLS"]
MAX_LINK_ROWS = _C["SQ_MAP_MAX_LINK_ROWS"]                  # rows one average-linkage problem may have
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


# ---------------------------------------------------------------------------------------------------------------------
# the cluster map: sns.clustermap(corrdf) of gbm_celltype_analysis.py:81,145 without the figure
# ---------------------------------------------------------------------------------------------------------------------
def _observations(A, what):
    """A f64 device tensor [K, M] or [B, K, M] -> ([B, K, M] view whose problems are K rows of leading dimension ld, B, K, M,
    ld, whether a batch was given)."""
    _on_device(A, what)
    if A.dtype != torch.float64:
        raise ValueError(f"{what}: dtype {A.dtype}, expected torch.float64")
    if A.dim() not in (2, 3):
        raise ValueError(f"{what}: a [K, M] matrix or a [B, K, M] batch is expected, got shape {tuple(A.shape)}")
    batched = A.dim() == 3
    t = A if batched else A.unsqueeze(0)
    B, K, M = (int(s) for s in t.shape)
    if B > 0 and K > 0 and M > 0:
        rows_ok = t.stride(2) == 1 and (K == 1 or t.stride(1) >= M)
        if not (rows_ok and (B == 1 or K == 1 or t.stride(0) == K * t.stride(1))):
            t = t.contiguous()
    ld = max(int(t.stride(1)), M, 1) if K > 1 and M > 0 else max(M, 1)
    return t, B, K, M, ld, batched


def _distances(t, B, K, M, ld, status):
    L = _lib.lib()
    need = int(L.sq_map_row_distances_workspace_bytes(B, K, M))
    dist = _empty(torch.float64, t.device, *((B, K, K) if need else (1, 1, 1)))     # a refused K may be too many rows to square
    src = t if t.numel() else _empty(torch.float64, t.device, 1)
    _call(L.sq_map_row_distances, t.device, src, B, K, M, ld, dist, status, workspace=need)
    return dist


def _raise_not_finite(what, dist_status):
    """dist_status: the downloaded int32 [B] words of sq_map_row_distances."""
    bad = np.nonzero(dist_status)[0]
    if bad.size:
        b = int(bad[0])
        where = f" of problem {b}" if dist_status.size > 1 else ""
        raise ValueError(f"{what}: row {int(dist_status[b]) - 1}{where} has a distance that is not finite (a NaN or infinite entry; a constant "
                         "gene makes its row and column of a correlation matrix NaN)")


def row_distances(A):
    """``scipy.spatial.distance.pdist(A, 'euclidean')`` as a square matrix, bit-equal to scipy: A f64 device tensor [K, M] (K
    observations of M features; rows may be a view of a wider table) or a batch [B, K, M] -> f64 [K, K] or [B, K, K],
    symmetric with an exactly-zero diagonal.  Per pair the features are summed in ascending order, product and sum rounded
    separately.  2 <= K <= MAX_LINK_ROWS.  A distance that is not finite raises ValueError naming the first such row."""
    _lib.require_gpu()
    t, B, K, M, ld, batched = _observations(A, "row_distances")
    status = _empty(torch.int32, t.device, B)
    dist = _distances(t, B, K, M, ld, status)
    _raise_not_finite("row_distances", status.cpu().numpy())
    return dist if batched else dist[0]


def linkage_average(A):
    """``Z = scipy.cluster.hierarchy.linkage(A, method='average', metric='euclidean')`` and ``leaves_list(Z)`` (the order
    ``dendrogram(Z, no_plot=True)['leaves']``, what seaborn's clustermap reorders by), bit-equal to scipy, ties and zero
    distances included.  A f64 device tensor [K, M] or a batch [B, K, M]; returns (Z f64 [K-1, 4], leaves int32 [K]) on the
    device, with a leading B for a batch (a batch equals the single calls byte for byte).  2 <= K <= MAX_LINK_ROWS: above
    it the library refuses (SequoiaHipArgError).  A distance that is not finite raises ValueError naming the first such
    row, as scipy raises; the status words are read once, after both launches."""
    _lib.require_gpu()
    t, B, K, M, ld, batched = _observations(A, "linkage_average")
    L = _lib.lib()
    status = _empty(torch.int32, t.device, 2, B)                # row 0: the distances' words, row 1: the linkage's
    dist = _distances(t, B, K, M, ld, status[0])
    need = int(L.sq_map_linkage_average_workspace_bytes(B, K))
    Z = _empty(torch.float64, t.device, *((B, K - 1, 4) if need else (1, 1, 4)))
    leaves = _empty(torch.int32, t.device, *((B, K) if need else (1, 1)))
    _call(L.sq_map_linkage_average, t.device, dist, B, K, status[0], Z, leaves, status[1], workspace=need)
    words = status.cpu().numpy()
    _raise_not_finite("linkage_average", words[0])
    if words[1].any():
        b = int(np.nonzero(words[1])[0][0])
        why = {_C["SQ_LINK_SEARCH_BOUND"]: "more than 3 (K - 1) nearest-neighbour searches",
               _C["SQ_LINK_BAD_DISTANCE"]: "a search met a distance that is NaN, infinite or negative"}.get(int(words[1][b]), "unknown status")
        raise _lib.SequoiaHipError(f"linkage_average: problem {b} ended with status {int(words[1][b])} ({why})")
    return (Z, leaves) if batched else (Z[0], leaves[0])


def cluster_order(matrix, device="cuda:0", return_linkage=False):
    """The rows and columns of a square symmetric matrix in the leaf order of the average linkage of its rows: what
    ``sns.clustermap(matrix)`` draws (seaborn clusters rows and columns separately; of a symmetric matrix both are this one
    linkage).  matrix: a DataFrame (uploaded to ``device``) -> (leaf order as an int array, the reordered DataFrame); or an
    f64 device tensor [K, K] -> (int32 leaves, ``matrix[leaves][:, leaves]``) on the device.  return_linkage: Z comes third.
    The matrix must be symmetric bit for bit (ValueError otherwise: the one order would not serve both axes)."""
    frame = None if torch.is_tensor(matrix) else matrix
    M = matrix if frame is None else torch.as_tensor(np.ascontiguousarray(frame.values, dtype=np.float64)).to(device)
    if M.dim() != 2 or M.shape[0] != M.shape[1]:
        raise ValueError(f"cluster_order: a square matrix is expected, got shape {tuple(M.shape)}")
    if M.dtype != torch.float64:
        raise ValueError(f"cluster_order: dtype {M.dtype}, expected torch.float64")
    if not torch.equal(M.contiguous().view(torch.int64), M.t().contiguous().view(torch.int64)):
        raise ValueError("cluster_order: the matrix is not symmetric bit for bit")
    Z, leaves = linkage_average(M)
    if frame is None:
        idx = leaves.to(torch.int64)
        out = (leaves, M[idx][:, idx])
    else:
        order = leaves.cpu().numpy()
        out = (order, frame.iloc[order, order])
    return out + (Z,) if return_linkage else out
