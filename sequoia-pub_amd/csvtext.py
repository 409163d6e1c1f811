"""The spatial prediction table written as CSV from the device -- the tail of the reference's spatial_vis/visualize.py
(:286-304): per gene and fold a column, per gene the fold mean, ``res_df.to_csv`` (csrc/csvtext.hip, csrc/fmt_core.h;
include/sequoia_hip.h, "CSV text").  ``cli.visualize --table device`` is the caller.

What is pinned, byte for byte, to pandas and numpy:
    fold mean   ``DataFrame.mean(axis=1)`` of float32 columns: a float32, the folds added in order in fp32 from +0.0 with
                NaN counting as +0.0, divided by the fp32 count of the values that are not NaN; no value gives NaN.
    rows        ``DataFrame.to_csv()`` with default arguments on Linux for an int64 index, int64 columns and float32
                columns: cells joined by ',', rows ended by '\\n', int64 as plain decimal, float32 as
                ``ndarray.astype(str)`` writes it, NaN as the empty cell.
    header      written by pandas itself from the empty frame, so quoting of odd column names is pandas'.
Left out: ``float_format``, ``decimal``, ``sep``, quoting options, another ``na_rep``, float64 columns, any index that is
not int64.  Tensors live on the device and there is no CPU fallback."""
import time

import numpy as np
import pandas as pd
import torch

from . import _lib
from ._abi import CONSTANTS as _C
from ._tables import _on_device, call as _call

MAX_TILES = 262144                        # rows of a table, as in the other slide analytics
MAX_CELL_BYTES = _C["SQ_CSV_MAX_CELL_BYTES"]
MAX_CELLS = _C["SQ_CSV_MAX_CELLS"]
MAX_FOLDS = _C["SQ_CSV_MAX_FOLDS"]
TEXT_BUDGET = 256 << 20                   # bytes of text per chunk: one device buffer and one pinned buffer of that size
SMALL_FRAME_CELLS = 1 << 22               # up to this many cells write_prediction_table also returns the frame


def fold_mean(x, out=None):
    """x: f32 [F, n, G] on the device (last dimension dense) -> f32 [n, G], ``DataFrame.mean(axis=1)`` over the folds of
    every (row, gene) bit for bit (module docstring).  ``out``: an f32 [n, G] device view to write to (its rows may be
    strided: columns of a wider table)."""
    _on_device(x, "fold_mean: x")
    if x.dtype != torch.float32 or x.dim() != 3:
        raise ValueError(f"fold_mean: x is {x.dtype} of shape {tuple(x.shape)}, expected float32 [F, n, G]")
    F, n, G = (int(s) for s in x.shape)
    if not 1 <= F <= MAX_FOLDS:
        raise ValueError(f"fold_mean: {F} folds, must be in 1..{MAX_FOLDS}")
    if out is None:
        out = torch.empty(n, G, dtype=torch.float32, device=x.device)
    _on_device(out, "fold_mean: out")
    if out.dtype != torch.float32 or tuple(out.shape) != (n, G) or out.device != x.device:
        raise ValueError(f"fold_mean: out is {out.dtype} {tuple(out.shape)} on {out.device}, expected float32 {(n, G)} on {x.device}")
    if n == 0 or G == 0:
        return out
    if x.stride(2) != 1 or (n > 1 and x.stride(1) < G):
        x = x.contiguous()
    if out.stride(1) != 1 or (n > 1 and out.stride(0) < G):
        raise ValueError(f"fold_mean: out has strides {out.stride()}; its rows must be dense")
    _lib.require_gpu()
    _call("sq_fold_mean_f32", x.device, x, F, x.stride(0) if F > 1 else 0, n, G, x.stride(1) if n > 1 else G, out, out.stride(0) if n > 1 else G)
    return out


def _parts(index, ints, floats, what):
    """The three tables of a frame as the library takes them: (index int64 [n], ints int64 [n, n_int] dense, floats f32
    [n, n_f32] with dense rows, ld of floats)."""
    for name, t, dt in (("index", index, torch.int64), ("ints", ints, torch.int64), ("floats", floats, torch.float32)):
        _on_device(t, f"{what}: {name}")
        if t.dtype != dt:
            raise ValueError(f"{what}: {name} has dtype {t.dtype}, expected {dt}")
    if index.dim() != 1 or ints.dim() != 2 or floats.dim() != 2 or ints.shape[0] != index.shape[0] or floats.shape[0] != index.shape[0]:
        raise ValueError(f"{what}: index {tuple(index.shape)}, ints {tuple(ints.shape)}, floats {tuple(floats.shape)}: expected [n], [n, n_int], [n, n_f32]")
    if not (index.device == ints.device == floats.device):
        raise _lib.SequoiaHipError(f"{what}: index is on {index.device}, ints on {ints.device}, floats on {floats.device}; all must be on one device")
    n, n_f32 = int(floats.shape[0]), int(floats.shape[1])
    if n_f32 and (floats.stride(1) != 1 or (n > 1 and floats.stride(0) < n_f32)):
        floats = floats.contiguous()
    ld = int(floats.stride(0)) if (n > 1 and n_f32) else max(n_f32, 1)
    return index.contiguous(), ints.contiguous(), floats, ld


def chunk_rows_for(n_int, n_f32, budget=TEXT_BUDGET):
    """Rows per format call so that the text of a chunk cannot exceed `budget` bytes (every cell at its longest,
    SQ_CSV_MAX_CELL_BYTES with its separator) nor the library's cell limit; at least one row."""
    cells = 1 + int(n_int) + int(n_f32)
    return int(max(1, min(int(budget) // (MAX_CELL_BYTES * cells), MAX_CELLS // cells)))


class RowFormatter:
    """The device side of the writer for one table: the text buffer, the row-offset table, the scalars and the workspace,
    allocated once for chunks of at most `chunk_rows` rows and reused by every ``format`` call."""

    def __init__(self, index, ints, floats, chunk_rows=None, budget=TEXT_BUDGET):
        self.index, self.ints, self.floats, self.ld = _parts(index, ints, floats, "RowFormatter")
        self.n, self.n_int, self.n_f32 = int(index.shape[0]), int(ints.shape[1]), int(floats.shape[1])
        if self.n > MAX_TILES:
            raise ValueError(f"RowFormatter: {self.n} rows, at most {MAX_TILES}")
        if chunk_rows is not None and int(chunk_rows) < 1:
            raise ValueError(f"RowFormatter: chunk_rows = {chunk_rows}, must be at least 1")
        rows = chunk_rows_for(self.n_int, self.n_f32, budget) if chunk_rows is None else int(chunk_rows)
        self.chunk_rows = max(1, min(rows, self.n, MAX_CELLS // (1 + self.n_int + self.n_f32)))
        self.capacity = self.chunk_rows * MAX_CELL_BYTES * (1 + self.n_int + self.n_f32)
        dev = index.device
        _lib.require_gpu()
        self.text = torch.empty(self.capacity, dtype=torch.uint8, device=dev)
        self.row_offsets = torch.empty(self.chunk_rows + 1, dtype=torch.int64, device=dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(_lib.need(_lib.lib().sq_csv_format_workspace_bytes, self.chunk_rows, self.n_int, self.n_f32),
                                     dtype=torch.uint8, device=dev)

    def format(self, lo, hi, capacity=None):
        """Rows lo .. hi - 1 into ``self.text`` (asynchronous).  ``self.total``, ``self.status`` and
        ``self.row_offsets[: hi - lo + 1]`` are the call's results; ``capacity``: a smaller bound than the buffer's."""
        lo, hi = int(lo), int(hi)
        if not (0 <= lo < hi <= self.n and hi - lo <= self.chunk_rows):
            raise ValueError(f"RowFormatter.format: rows {lo}..{hi} of {self.n}, at most {self.chunk_rows} per call")
        cap = self.capacity if capacity is None else int(capacity)
        if not 0 <= cap <= self.capacity:
            raise ValueError(f"RowFormatter.format: capacity {cap} outside 0..{self.capacity}")
        _call("sq_csv_format_rows", self.index.device, self.index, self.ints if self.n_int else None, self.n_int,
              self.floats if self.n_f32 else None, self.n_f32, self.ld, lo, hi, self.text, cap, self.row_offsets, self.total, self.status,
              workspace=self.workspace)

    def result(self):
        """Waits for the last ``format``: its byte count; an overflow of the capacity raises."""
        total, status = int(self.total.item()), int(self.status.item())
        if status != _C["SQ_CSV_OK"]:
            raise _lib.SequoiaHipError(f"csv text: the rows need {total} bytes, the buffer holds fewer (status {status})")
        return total


def write_rows(f, index, ints, floats, chunk_rows=None, budget=TEXT_BUDGET):
    """Append the rows of the frame (index int64 [n], ints int64 [n, n_int], floats f32 [n, n_f32], all on one device) to
    the binary file object `f` as ``DataFrame.to_csv(header=False)`` writes them: chunks of rows formatted on the device
    into one text buffer of at most `budget` bytes, downloaded through one pinned buffer, written.  Returns the seconds
    spent per stage: {"format", "download", "write"} and the "bytes" written."""
    spent = {"format": 0.0, "download": 0.0, "write": 0.0, "bytes": 0}
    if int(index.shape[0]) == 0:
        _parts(index, ints, floats, "write_rows")
        return spent
    fm = RowFormatter(index, ints, floats, chunk_rows=chunk_rows, budget=budget)
    pinned = torch.empty(fm.capacity, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    dev = index.device
    for lo in range(0, fm.n, fm.chunk_rows):
        t0 = time.perf_counter()
        fm.format(lo, min(fm.n, lo + fm.chunk_rows))
        total = fm.result()
        t1 = time.perf_counter()
        pinned[:total].copy_(fm.text[:total], non_blocking=True)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        f.write(memoryview(host)[:total])
        t3 = time.perf_counter()
        spent["format"] += t1 - t0
        spent["download"] += t2 - t1
        spent["write"] += t3 - t2
        spent["bytes"] += total
    return spent


def header_line(names, index=None):
    """The header ``to_csv`` writes for these columns (and this index, for its name), by pandas from the empty frame."""
    return pd.DataFrame(columns=list(names), index=None if index is None else index[:0]).to_csv().encode()


def frame_refusal(df, names):
    """Why the device writer cannot take this frame and these further column names -- a sentence -- or None."""
    if df.index.dtype != np.int64:
        return f"the index has dtype {df.index.dtype}, not int64"
    bad = [f"{c} ({df[c].dtype})" for c in df.columns if df[c].dtype != np.int64]
    if bad:
        return "the coordinate columns are not all int64: " + ", ".join(bad)
    every = [str(c) for c in df.columns] + list(names)
    if len(set(every)) != len(every):
        return "two columns would share a name"
    return None


def write_prediction_table(path, df, table, names, budget=TEXT_BUDGET, chunk_rows=None, small=SMALL_FRAME_CELLS):
    """``res_df.to_csv(path)`` for res_df = the int64 frame `df` (RangeIndex or any int64 index) followed by the float32
    columns `names` of the device table [len(df), len(names)], byte for byte, without the frame: pandas writes the header
    line, the rows are formatted on the device.  Returns (res_df or None, spent): the frame itself only when it has at
    most `small` cells -- a table of 50 000 tiles x 1 500 columns would be 300 MB of host columns nobody reads, the file is the
    result --, and the seconds per stage of ``write_rows``."""
    why = frame_refusal(df, names)
    if why:
        raise ValueError(f"write_prediction_table: {why}")
    n = len(df)
    if tuple(table.shape) != (n, len(names)):
        raise ValueError(f"write_prediction_table: the table has shape {tuple(table.shape)}, expected {(n, len(names))}")
    dev = table.device
    index = torch.from_numpy(np.ascontiguousarray(df.index.values, dtype=np.int64)).to(dev)
    ints = torch.from_numpy(np.ascontiguousarray(df.values, dtype=np.int64).reshape(n, len(df.columns))).to(dev)
    with open(path, "wb") as f:
        f.write(header_line([*df.columns, *names], df.index))
        spent = write_rows(f, index, ints, table, chunk_rows=chunk_rows, budget=budget)
    res = None
    if n * (len(df.columns) + len(names)) <= small:
        host = table.cpu().numpy()
        res = pd.concat([df, pd.DataFrame({c: host[:, k] for k, c in enumerate(names)}, index=df.index, columns=list(names))], axis=1)
    return res, spent
