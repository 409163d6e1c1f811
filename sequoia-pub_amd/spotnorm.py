"""Raw spatial-transcriptomics spots read from an ``.h5ad`` file and normalised on the device -- the first lines of the
reference's spatial_vis/get_emd.py (:148-155): ``sc.read_h5ad``, ``sc.pp.normalize_total(adata, inplace=True)``,
``sc.pp.log1p``, ``sc.pp.scale`` and ``adata[:, gene].X`` (csrc/spotnorm.hip; include/sequoia_hip.h, "Spot normalisation").

The contract, everything in f64 over X [n_spots, n_genes] in CSR with non-negative finite values:
    counts        c_i = sum_j X_ij                                    (normalize_total: counts per cell)
    target        after = np.median(c[c > 0]); no spot with counts is an error
    size factor   s_i = (c_i + (c_i == 0)) / after, v_ij = X_ij / s_i   (scanpy's two divisions in scanpy's order)
    log           l_ij = log1p(v_ij)
    scale         m_j = sum_i l_ij / n; var_j = sum_i (l_ij - m_j)^2 / (n - 1), two-pass; sd_j = sqrt(var_j), 0 -> 1;
                  z_ij = (l_ij - m_j) / sd_j; the sums run over all n spots, zeros included; n >= 2
Counts, target and size factors use every gene; log and scale are per column, so only the requested genes are made.
No floating-point atomics and every sum in a fixed order: two calls give the same bytes.  With integer counts (what the
reference's files hold) c, after, s and v equal numpy's and scipy's bit for bit.

This is NOT scanpy digit for digit: scanpy works in the matrix's own dtype, usually float32, and none of scanpy, anndata
and h5py was at hand to compare with; the contract is stated here and tested against an extended-precision evaluation of
itself.  Left out: ``exclude_highly_expressed``, ``target_sum``, ``max_value``, layers and backed mode.  A gene that is
constant and non-zero after the log (possible only if all spots have equal totals) gets a rounding-noise ``sd`` and a
noise ``z``, as in scanpy; an all-zero gene gives z = 0 exactly.

Tensors live on the device and there is no CPU fallback; ``read_h5ad`` is host work (h5lite.py on libhdf5, scipy)."""
import numpy as np
import torch

from . import _lib
from ._abi import CONSTANTS as _C
from ._tables import _on_device, call as _call, columns as _columns, empty as _empty, vector as _vector
from .gtalign import MAX_SPOTS

MAX_GENES = _C["SQ_SN_MAX_GENES"]
MAX_NNZ = _C["SQ_SN_MAX_NNZ"]
MAX_CELLS = _C["SQ_SN_MAX_CELLS"]
_KINDS = {torch.float32: _C["SQ_SN_DATA_F32"], torch.float64: _C["SQ_SN_DATA_F64"], torch.int32: _C["SQ_SN_DATA_I32"]}
_STATUS = ((_C["SQ_SN_BAD_INDPTR"], "indptr is not non-decreasing within 0..nnz"),
           (_C["SQ_SN_BAD_INDEX"], "a column index is outside [0, n_genes)"),
           (_C["SQ_SN_BAD_ORDER"], "a row's column indices are not strictly increasing (sort the indices and sum the duplicates first)"),
           (_C["SQ_SN_BAD_VALUE"], "a value is negative or not finite"))


def _csr(data, indices, indptr, n_genes, what):
    for name, t in (("data", data), ("indices", indices), ("indptr", indptr)):
        _on_device(t, f"{what}: {name}")
    if not (data.device == indices.device == indptr.device):
        raise _lib.SequoiaHipError(f"{what}: data is on {data.device}, indices on {indices.device}, indptr on {indptr.device}; all must be on one device")
    if data.dtype not in _KINDS:
        raise ValueError(f"{what}: data has dtype {data.dtype}, expected one of {[str(d) for d in _KINDS]}")
    if indices.dtype not in (torch.int32, torch.int64) or indptr.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: indices ({indices.dtype}) and indptr ({indptr.dtype}) must be int32 or int64")
    if not isinstance(n_genes, (int, np.integer)) or isinstance(n_genes, bool):
        raise ValueError(f"{what}: n_genes = {n_genes!r}, must be an integer")
    if not 0 <= int(n_genes) < 2 ** 31 or data.numel() >= 2 ** 31 or indptr.numel() > 2 ** 31:
        raise ValueError(f"{what}: n_genes = {int(n_genes)}, nnz = {data.numel()}, n_spots = {indptr.numel() - 1}: an extent does not fit 32 bits "
                         f"(limits: {MAX_SPOTS} spots, {MAX_GENES} genes, {MAX_NNZ} entries)")
    if data.dim() != 1 or indices.shape != data.shape:
        raise ValueError(f"{what}: data {tuple(data.shape)} and indices {tuple(indices.shape)} must be vectors of one length")
    if indptr.dim() != 1 or indptr.numel() < 1:
        raise ValueError(f"{what}: indptr has shape {tuple(indptr.shape)}, expected (n_spots + 1,)")
    nnz, n_spots = int(data.numel()), int(indptr.numel()) - 1
    if indices.dtype == torch.int64 and nnz and bool(((indices < 0) | (indices >= int(n_genes))).any()):
        raise ValueError(f"{what}: a column index is outside [0, n_genes = {int(n_genes)})")
    ends = indptr[[0, -1]].cpu().tolist()
    if ends != [0, nnz]:
        raise ValueError(f"{what}: indptr runs from {ends[0]} to {ends[1]}, expected 0 to nnz = {nnz}")
    return data.contiguous(), _vector(indices, torch.int32, f"{what}: indices"), _vector(indptr, torch.int64, f"{what}: indptr"), n_spots, nnz


def normalize_spots(data, indices, indptr, n_genes, cols=None, scale=True, return_stats=False):
    """get_emd.py:148-155 for the CSR matrix (data, indices, indptr) of [n_spots, n_genes] raw counts on the device.
    data: f32, f64 or int32 [nnz]; indices: int32 (or int64) [nnz], strictly increasing within a row; indptr: int64 (or
    int32) [n_spots + 1]; cols: which genes, in which order, repeats allowed (None: all).  Returns f64 [n_spots, C] on
    the device: z, or the log1p values L when scale is False.  return_stats: also a dict with ``counts`` f64 [n_spots],
    ``after`` (float), ``size_factors`` f64 [n_spots], ``mean`` and ``std`` f64 [C] (of L, whether scaled or not).
    Refused with ValueError: an unsorted row, an index out of range, a negative or non-finite value, no spot with
    counts, fewer than two spots when the scale step runs; sizes beyond the library's limits carry its message."""
    what = "normalize_spots"
    data, indices, indptr, n_spots, nnz = _csr(data, indices, indptr, n_genes, what)
    n_genes = int(n_genes)
    _lib.require_gpu()
    dev = data.device
    col_t, C = _columns(cols, max(n_genes, 0), dev, what)
    need_scale = bool(scale) or bool(return_stats)
    if need_scale and n_spots < 2:
        raise ValueError(f"{what}: n_spots = {n_spots}, the scale step needs at least 2 spots (ddof 1)")
    L_ = _lib.lib()
    kind = _KINDS[data.dtype]
    counts = _empty(torch.float64, dev, n_spots)
    status = torch.zeros(2, dtype=torch.int32, device=dev)          # [status word, positive spots]
    after = torch.zeros(1, dtype=torch.float64, device=dev)
    _call(L_.sq_spot_counts, dev, data, kind, indices, indptr, n_spots, n_genes, nnz, counts, status)
    _call(L_.sq_spot_target, dev, counts, n_spots, after, status[1:], workspace=int(L_.sq_spot_target_workspace_bytes(n_spots)))
    word, positive = status.cpu().tolist()                          # the one synchronisation: nothing is built on a bad matrix
    for bit, text in _STATUS:
        if word & bit:
            raise ValueError(f"{what}: {text}")
    if positive == 0:
        raise ValueError(f"{what}: no spot has counts: the median of the positive totals does not exist")
    out = _empty(torch.float64, dev, n_spots, C)
    _call(L_.sq_spot_log_columns, dev, data, kind, indices, indptr, n_spots, n_genes, nnz, counts, after, col_t, C, out)
    mean = std = None
    if need_scale:
        mean, std = _empty(torch.float64, dev, C), _empty(torch.float64, dev, C)
        _call(L_.sq_spot_scale, dev, out, n_spots, max(C, 1), C, mean, std, int(bool(scale)))
    if not return_stats:
        return out
    return out, dict(counts=counts, after=float(after.item()), size_factors=(counts + (counts == 0)) / after, mean=mean, std=std)


# ---------------------------------------------------------------------------------------------------------------------
# .h5ad
# ---------------------------------------------------------------------------------------------------------------------
def _text(v):
    return v.decode("utf-8") if isinstance(v, bytes) else str(v)


def _numeric_obs(f, path, name):
    full = f"obs/{name}"
    if f"obs/__categories/{name}" in f:
        raise ValueError(f"read_h5ad: {path}: obs/{name} is categorical (codes with obs/__categories/{name}); numeric coordinates are expected")
    if full not in f:
        raise ValueError(f"read_h5ad: {path}: obs has no '{name}' (found {sorted(f['obs'].keys())[:12]})")
    if f.kind(full) != "dataset":
        enc = _text(f[full].attrs.get("encoding-type", "a group"))
        raise ValueError(f"read_h5ad: {path}: obs/{name} is {enc}, not a numeric dataset (a categorical coordinate is not read)")
    if f.type_class(full) not in ("integer", "float"):
        raise ValueError(f"read_h5ad: {path}: obs/{name} holds {f.type_class(full)} values; numeric coordinates are expected")
    return np.asarray(f[full][...], dtype=np.float64)


def read_h5ad(path):
    """The raw matrix, spot coordinates and gene names of an anndata file (the on-disk format of anndata 0.7 and later)
    -> (scipy.sparse.csr_matrix [n_spots, n_genes] in canonical form, x f64 [n_spots], y f64 [n_spots], gene names, a
    list of str).  ``X`` is a group with the attributes ``encoding-type`` (csr_matrix or csc_matrix; ``h5sparse_format``
    in 0.7 files) and ``shape`` and the datasets data, indices, indptr, or a dense dataset; ``obs/x`` and ``obs/y`` are
    numeric datasets; the gene names are the dataset that the ``_index`` attribute of ``var`` names (default ``_index``),
    variable- or fixed-length UTF-8.  CSC and dense input is converted and the CSR made canonical (duplicates summed,
    indices sorted) with scipy on the host.  Refused, with what was found: ``obs`` or ``var`` as a dataset (the legacy
    compound layout), a categorical x or y, a missing index, a file that holds only ``raw``."""
    import scipy.sparse as sp
    from . import h5lite
    with h5lite.File(path, "r") as f:
        if "X" not in f:
            if "raw" in f and "raw/X" in f:
                raise ValueError(f"read_h5ad: {path} has no X, only raw/X: a raw-only file is not read (found {sorted(f.keys())})")
            raise ValueError(f"read_h5ad: {path} has no X (found {sorted(f.keys())})")
        for table in ("obs", "var"):
            if table not in f:
                raise ValueError(f"read_h5ad: {path} has no {table} (found {sorted(f.keys())})")
            if f.kind(table) != "group":
                raise ValueError(f"read_h5ad: {path}: {table} is a dataset of {f.type_class(table)} type, not a group: the legacy "
                                 f"compound-dataset layout (anndata before 0.7) is not read")
        x, y = _numeric_obs(f, path, "x"), _numeric_obs(f, path, "y")
        index = _text(f["var"].attrs.get("_index", "_index"))
        if f"var/{index}" not in f or f.kind(f"var/{index}") != "dataset":
            raise ValueError(f"read_h5ad: {path}: var has no index dataset '{index}' (found {sorted(f['var'].keys())[:12]})")
        if f.type_class(f"var/{index}") != "string":
            raise ValueError(f"read_h5ad: {path}: var/{index} holds {f.type_class(f'var/{index}')} values; gene names are expected")
        genes = [str(g) for g in f[f"var/{index}"][...]]
        if f.kind("X") == "group":
            X = f["X"]
            attrs = X.attrs
            enc = _text(attrs.get("encoding-type", attrs.get("h5sparse_format", "")))
            enc = enc if enc.endswith("_matrix") else enc + "_matrix"
            shape = attrs.get("shape", attrs.get("h5sparse_shape"))
            if enc not in ("csr_matrix", "csc_matrix") or shape is None or len(shape) != 2:
                raise ValueError(f"read_h5ad: {path}: X is a group with encoding-type {enc!r} and shape {shape!r}; csr_matrix or csc_matrix "
                                 f"with a 2-element shape is expected")
            missing = [k for k in ("data", "indices", "indptr") if k not in X]
            if missing:
                raise ValueError(f"read_h5ad: {path}: X lacks {missing} (found {sorted(X.keys())})")
            parts = (X["data"][...], X["indices"][...], X["indptr"][...])
            shape = (int(shape[0]), int(shape[1]))
            m = (sp.csr_matrix if enc == "csr_matrix" else sp.csc_matrix)(parts, shape=shape)
        else:
            if f.type_class("X") not in ("integer", "float"):
                raise ValueError(f"read_h5ad: {path}: X holds {f.type_class('X')} values; numbers are expected")
            dense = np.asarray(f["X"][...])
            if dense.ndim != 2:
                raise ValueError(f"read_h5ad: {path}: the dense X has shape {dense.shape}; [n_spots, n_genes] is expected")
            m = sp.csr_matrix(dense)
    m = sp.csr_matrix(m)                                    # CSC -> CSR
    m.sum_duplicates()
    m.sort_indices()
    if m.shape != (len(x), len(genes)) or len(y) != len(x):
        raise ValueError(f"read_h5ad: {path}: X is {m.shape}, obs has {len(x)} x and {len(y)} y, var {len(genes)} names")
    return m, x, y, genes


def _data_tensor(data):
    """CSR values as one of the three dtypes the library reads: integers up to 32 bits as int32, f32 as is, else f64."""
    if data.dtype.kind in "iu" and (data.dtype.itemsize < 4 or data.dtype == np.int32):
        return data.astype(np.int32)
    return data if data.dtype == np.float32 else data.astype(np.float64)


def csr_to_device(csr, device):
    """(data, indices, indptr) of a canonical scipy CSR matrix as device tensors for ``normalize_spots``."""
    return (torch.as_tensor(np.ascontiguousarray(_data_tensor(csr.data))).to(device),
            torch.as_tensor(np.ascontiguousarray(csr.indices, dtype=np.int32)).to(device),
            torch.as_tensor(np.ascontiguousarray(csr.indptr, dtype=np.int64)).to(device))


def spots_from_h5ad(path, genes, device):
    """``read_h5ad`` and ``normalize_spots`` for the requested genes -> (spot_x, spot_y, expr) on the device: f64 [n_spots],
    f64 [n_spots] and f64 [n_spots, len(genes)], what ``gtalign.align_ground_truth`` takes.  The normalisation runs once
    for all genes (the reference redoes it per gene).  A requested gene that the file lacks, or holds more than once
    (anndata would return two columns), is refused."""
    genes = list(genes)
    if not genes:
        raise ValueError("spots_from_h5ad: no genes requested")
    csr, x, y, names = read_h5ad(path)
    where = {}
    for j, g in enumerate(names):
        where.setdefault(g, []).append(j)
    missing = [g for g in genes if g not in where]
    if missing:
        raise ValueError(f"spots_from_h5ad: {path} has no genes {missing[:8]}")
    twice = [g for g in genes if len(where[g]) > 1]
    if twice:
        raise ValueError(f"spots_from_h5ad: the gene names {twice[:8]} are duplicated in {path}: columns {[where[g] for g in twice[:8]]}")
    device = torch.device(device)
    data, indices, indptr = csr_to_device(csr, device)
    expr = normalize_spots(data, indices, indptr, csr.shape[1], cols=[where[g][0] for g in genes])
    return torch.as_tensor(x).to(device), torch.as_tensor(y).to(device), expr
