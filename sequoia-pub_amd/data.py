"""Data feed -- host-side counterpart of /root/reference/src/read_data.py:12-56 (``SuperTileRNADataset``) and
/root/reference/src/utils.py:10-41,79-110 (``custom_collate_fn``, ``filter_no_features``, ``patient_kfold``).
Pure host logic (pandas / numpy / sklearn splitters); the tensors it yields feed the HIP path.

Same inputs, outputs and file rules as the reference; organised around whole-frame passes: store paths, names and
targets are materialised once per dataset, the feature filter scans each project directory once into a
name -> usable map, and the k-fold split is a patient -> role table expanded to row indices.

The opt-in device-resident feed (``CohortTable``, ``ResidentLoader``; ``--feed resident`` of the training and inference CLIs) reads
the cohort once, keeps it on the device and gathers every batch there (csrc/cohort.hip: ``sq_cohort_gather``): the same batches in
the same order as the loader path, which stays the default."""
import os

import numpy as np
import pandas as pd
import torch
from torch.utils.data import Dataset

from . import store


def slide_store_path(features_path, project, wsi_file_name):
    """``<features_path>/<project>/<WSI>/<WSI>.h5``; TCGA names lose their ``.svs`` suffix, GTEx paths keep it
    (read_data.py:45-46)."""
    path = os.path.join(features_path, project, wsi_file_name, wsi_file_name + '.h5')
    return path if 'GTEX' in path else path.replace('.svs', '')


class SuperTileRNADataset(Dataset):
    """One item per reference-CSV row: (features f32 [100, D] or None, rna f32 [G], wsi_file_name, tcga_project)
    -- read_data.py:12-56.  ``feature_use`` names the dataset read per slide (the reference's ``__init__`` reads an
    undefined ``self.feature_use`` and ``__getitem__`` hard-codes ``'cluster_features'``; the intended behaviour
    -- predict_independent_dataset.py:54 passes it as third argument -- is implemented)."""

    def __init__(self, csv_path, features_path, feature_use="cluster_features", quick=None):
        self.csv_path = csv_path
        self.quick = quick
        self.features_path = features_path
        self.feature_use = feature_use
        self.data = pd.read_csv(csv_path) if isinstance(csv_path, str) else csv_path
        self.rna_cols = [c for c in self.data.columns if 'rna_' in c]
        self.num_genes = len(self.rna_cols)
        # whole-frame materialisation: no 20 823-column pandas row slice per item
        self._targets = self.data[self.rna_cols].to_numpy(dtype=np.float32)
        self._names = self.data['wsi_file_name'].to_numpy()
        self._projects = self.data['tcga_project'].to_numpy()
        self._paths = [slide_store_path(features_path, p, w) for p, w in zip(self._projects, self._names)]
        with store.File(self._paths[0], 'r') as f:
            self.feature_dim = f[self.feature_use][:].shape[1]

    def __len__(self):
        return len(self._paths)

    def _load(self, path):
        """The slide's token matrix, or None (with the reference's two prints) when the store cannot give it:
        such rows are dropped by the collate function (read_data.py:51-54)."""
        try:
            with store.File(path, 'r') as f:
                return torch.tensor(np.asarray(f[self.feature_use][:]), dtype=torch.float32)
        except Exception as e:
            print(e)
            print(path)
            return None

    def __getitem__(self, idx):
        return (self._load(self._paths[idx]), torch.from_numpy(self._targets[idx].copy()),
                self._names[idx], self._projects[idx])


def custom_collate_fn(batch):
    """utils.py:10-18: drop entries whose features failed to load, then default_collate (an all-bad batch
    collates to an empty list, which the loops skip: vit.py:159)."""
    usable = [item for item in batch if item[0] is not None]
    if not usable:
        return [], [], [], []
    return torch.utils.data.dataloader.default_collate(usable)


# ---------------------------------------------------------------------------------------------
# device-resident feed: the cohort read once, batches gathered on the device (csrc/cohort.hip)
# ---------------------------------------------------------------------------------------------
def cohort_gather(x_table, index=None, y_table=None, x_out=None, y_out=None):
    """Rows ``index`` of f32 CUDA tables ``x_table [S, ...]`` and ``y_table [S, ...]`` (None: features only) in one launch
    (``sq_cohort_gather``): returns ``(x [m, ...], y [m, ...] or None)``.  ``index``: int32 [m] on the tables' device, None for all
    rows in order; an index outside [0, S) gives zero rows.  ``x_out`` / ``y_out``: contiguous f32 tensors of those shapes to write
    into.  Asynchronous on the current stream; no CPU fallback."""
    from . import _lib
    _lib.require_gpu()
    tables = [t for t in (x_table, y_table) if t is not None]
    for t in tables:
        if not (torch.is_tensor(t) and t.is_cuda and t.device == x_table.device):
            raise _lib.SequoiaHipError("cohort_gather needs CUDA tensors on one device (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.shape[0] != x_table.shape[0]:
            raise ValueError(f"cohort_gather: a table must be contiguous float32 [{x_table.shape[0]}, ...], got {t.dtype} {tuple(t.shape)}")
    dev, S = x_table.device, x_table.shape[0]
    if index is None:
        m = S
    elif not (torch.is_tensor(index) and index.device == dev):
        raise _lib.SequoiaHipError("cohort_gather: index must be a tensor on the device of the tables")
    elif index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous():
        raise ValueError(f"cohort_gather: index must be contiguous int32 [m], got {index.dtype} {tuple(index.shape)}")
    else:
        m = index.shape[0]
    outs = []
    for t, out in ((x_table, x_out), (y_table, y_out)):
        if t is not None and out is None:
            out = torch.empty((m,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        elif t is None and out is not None:
            raise ValueError("cohort_gather: y_out without a y_table")
        elif t is not None and not (out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
                                    and tuple(out.shape) == (m,) + tuple(t.shape[1:])):
            raise ValueError(f"cohort_gather: an output must be contiguous float32 {(m,) + tuple(t.shape[1:])} on {dev}")
        outs.append(out)
    row_x, row_y = (0 if t is None else int(np.prod(t.shape[1:])) for t in (x_table, y_table))
    _lib.call("sq_cohort_gather", dev, x_table, y_table, S, row_x, row_y, index, m, outs[0], outs[1])
    return outs[0], outs[1]


class CohortTable:
    """A cohort's features and targets read ONCE: what ``SuperTileRNADataset`` over the same arguments returns item by item and
    epoch by epoch, as two host arrays ``x [S, tokens, D]`` and ``y [S, G]`` f32 with ``valid [S]``, ``names`` and ``projects``.
    A slide whose store cannot be read or lacks ``feature_use`` is invalid (its row of x stays zero; the exception and the path are
    printed here, once -- the loader path prints them every epoch) and is dropped from every batch of the run, as
    ``custom_collate_fn`` drops it.  A slide whose dataset has another shape than the first readable one is refused by name (the
    loader path fails in default_collate on the first batch that mixes two shapes).  Stores are read one after another on this
    thread (h5lite drives the system's HDF5 C library, which need not be thread-safe).

    ``to(device)`` uploads both arrays through one pinned buffer; datasets (folds, roles) are row subsets of the one table:
    ``ResidentLoader(table, rows, ...)``."""

    STAGING_BYTES = 256 << 20

    def __init__(self, csv_path, features_path, feature_use="cluster_features"):
        self.features_path, self.feature_use = features_path, feature_use
        data = pd.read_csv(csv_path) if isinstance(csv_path, str) else csv_path
        self.rna_cols = [c for c in data.columns if 'rna_' in c]
        self.num_genes = len(self.rna_cols)
        self.y = np.ascontiguousarray(data[self.rna_cols].to_numpy(dtype=np.float32))
        self.names = data['wsi_file_name'].to_numpy()
        self.projects = data['tcga_project'].to_numpy()
        self.paths = [slide_store_path(features_path, p, w) for p, w in zip(self.projects, self.names)]
        self.valid = np.zeros(len(self.paths), dtype=bool)
        self.x = None
        for i, path in enumerate(self.paths):
            try:
                with store.File(path, 'r') as f:
                    item = torch.tensor(np.asarray(f[feature_use][:]), dtype=torch.float32).numpy()      # SuperTileRNADataset._load
            except Exception as e:
                print(e)
                print(path)
                continue
            if self.x is None:
                if item.ndim != 2:
                    raise ValueError(f"CohortTable: {feature_use} of slide {self.names[i]} has shape {item.shape}, expected [tokens, D]")
                self.x = np.zeros((len(self.paths),) + item.shape, dtype=np.float32)
            elif item.shape != self.x.shape[1:]:
                raise ValueError(f"CohortTable: {feature_use} of slide {self.names[i]} has shape {item.shape}, the cohort's first "
                                 f"readable slide has {self.x.shape[1:]}: one table holds one shape")
            self.x[i] = item
            self.valid[i] = True
        if self.x is None:
            raise ValueError(f"CohortTable: none of the {len(self.paths)} slides has a readable {feature_use}")
        self.tokens, self.feature_dim = self.x.shape[1:]
        self.x_dev = self.y_dev = None

    def __len__(self):
        return len(self.paths)

    @property
    def nbytes(self):
        return self.x.nbytes + self.y.nbytes

    def to(self, device, max_bytes=None):
        """Upload x and y to ``device`` (kept as ``x_dev``, ``y_dev``) through one pinned buffer of at most STAGING_BYTES.  Tables
        larger than ``max_bytes`` (default: half of the device's free memory now) are refused before anything is allocated."""
        device = torch.device(device)
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(device)[0] // 2
        if self.nbytes > max_bytes:
            raise ValueError(f"CohortTable: the tables take {self.nbytes} bytes ({self.x.nbytes} of features, {self.y.nbytes} of targets), "
                             f"more than max_bytes = {int(max_bytes)}: keep the loader feed for this cohort or raise max_bytes")
        staging = torch.empty(max(1, min(self.STAGING_BYTES, max(self.x.nbytes, self.y.nbytes)) // 4), dtype=torch.float32).pin_memory()
        placed = []
        for host in (self.x, self.y):
            src = torch.from_numpy(host).reshape(-1)
            dst = torch.empty(src.numel(), dtype=torch.float32, device=device)
            for lo in range(0, src.numel(), staging.numel()):
                n = min(staging.numel(), src.numel() - lo)
                staging[:n].copy_(src[lo:lo + n])
                dst[lo:lo + n].copy_(staging[:n], non_blocking=True)
                torch.cuda.synchronize(device)                 # the one buffer is refilled next
            placed.append(dst.view(host.shape))
        self.x_dev, self.y_dev = placed
        return self

    def gather(self, index):
        """``(x [m, tokens, D], y [m, G])`` on the device: rows ``index`` (int32 [m] on the device) of the uploaded tables."""
        if self.x_dev is None:
            raise RuntimeError("CohortTable: call to(device) before gathering batches")
        return cohort_gather(self.x_dev, index, self.y_dev)


class RowIndex(Dataset):
    """The index-only dataset of n rows: item i is i.  What a sampler of the resident feed is built over."""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class ResidentLoader:
    """Batches of rows ``rows`` of an uploaded CohortTable, in the place of ``DataLoader(SuperTileRNADataset(frame.iloc[rows]),
    batch_size, shuffle, sampler, generator, collate_fn=custom_collate_fn)``: the same batches in the same order, with the same
    draws from ``generator`` and from the global torch RNG.  The order is not restated: it is what a DataLoader of the same
    arguments over ``RowIndex(len(rows))`` yields.  ``sampler`` (a DistributedSampler) is built over ``RowIndex(len(rows))``.
    Yields ``(x, y, names, projects)`` with x and y on the table's device; invalid rows are dropped, an all-invalid batch is
    ``([], [], [], [])``."""

    def __init__(self, table, rows, batch_size=1, shuffle=False, generator=None, sampler=None):
        self.table = table
        self.rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        self._order = torch.utils.data.DataLoader(RowIndex(len(self.rows)), batch_size=batch_size, shuffle=shuffle, sampler=sampler,
                                                  generator=generator, num_workers=0, collate_fn=list)

    @property
    def sampler(self):
        return self._order.sampler

    @property
    def batch_size(self):
        return self._order.batch_size

    def __len__(self):
        return len(self._order)

    def index_batches(self):
        """The host half: per batch the list of positions in ``rows``, as the DataLoader hands them to a dataset."""
        return iter(self._order)

    def __iter__(self):
        collate = torch.utils.data.dataloader.default_collate
        table = self.table
        if table.x_dev is None:
            raise RuntimeError("ResidentLoader: the table is not on a device: call table.to(device) first")
        for positions in self.index_batches():
            rows = self.rows[positions]
            rows = rows[table.valid[rows]]                     # custom_collate_fn: items whose features failed to load are dropped
            if rows.size == 0:
                yield [], [], [], []
                continue
            x, y = table.gather(torch.from_numpy(rows.astype(np.int32)).to(table.x_dev.device))
            names, projects = collate([(table.names[i], table.projects[i]) for i in rows])       # the containers default_collate makes
            yield [x, y, names, projects]


def _has_dataset(path, name):
    try:
        with store.File(path, "r") as f:
            return name in f.keys()
    except Exception:
        return False


def filter_no_features(df, feature_path, feature_name):
    """Rows of df whose slide has a readable store holding `feature_name` (utils.py:21-41).  A slide name that
    is unusable under ANY of the frame's projects is dropped everywhere, like the reference's remove-by-name."""
    print(f'Filtering WSIs that do not have {feature_name} features')
    usable = {}
    for proj in np.unique(df.tcga_project):
        for wsi in os.listdir(os.path.join(feature_path, proj)):
            ok = _has_dataset(os.path.join(feature_path, proj, wsi, wsi + '.h5'), feature_name)
            usable[wsi] = usable.get(wsi, True) and ok
    keep = df['wsi_file_name'].map(lambda w: usable.get(w, False)).to_numpy(dtype=bool)
    print(f'Original shape: {df.shape}')
    df = df[keep].reset_index(drop=True)
    print(f'New shape: {df.shape}')
    return df


def patient_kfold(dataset, n_splits=5, random_state=0, valid_size=0.1):
    """Patient-level cross-validation (utils.py:79-110): KFold(shuffle, random_state) over the sorted unique patient
    ids; `valid_size` of each fold's training patients (train_test_split, random_state=0) becomes the validation
    part.  Returns (train_idx, valid_idx, test_idx): per fold, ascending row indices."""
    from sklearn.model_selection import KFold, train_test_split
    patients, patient_of_row = np.unique(np.asarray(dataset.patient_id), return_inverse=True)
    TRAIN, VALID, TEST = 0, 1, 2
    folds = {TRAIN: [], VALID: [], TEST: []}
    for keep_pos, test_pos in KFold(n_splits, shuffle=True, random_state=random_state).split(patients):
        role = np.full(len(patients), TRAIN, dtype=np.int8)
        role[test_pos] = TEST
        if valid_size > 0:
            _, valid_pos = train_test_split(keep_pos, test_size=valid_size, random_state=0)
            role[valid_pos] = VALID
        row_role = role[patient_of_row]
        folds[TEST].append(np.flatnonzero(row_role == TEST))
        folds[TRAIN].append(np.flatnonzero(row_role == TRAIN))
        if valid_size > 0:
            folds[VALID].append(np.flatnonzero(row_role == VALID))
    return folds[TRAIN], folds[VALID], folds[TEST]


def shard_rows(n_rows, rank, world):
    """Contiguous slide range of one rank -- the reference's --start/--end parallelisation
    (compute_features_hdf5.py:80-85, kmean_features.py:56-61) chosen automatically per GPU."""
    per = (n_rows + world - 1) // world
    lo = min(n_rows, rank * per)
    return lo, min(n_rows, lo + per)
