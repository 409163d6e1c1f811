"""Cases of the device spot normalisation (sequoia_pub_amd.spotnorm, csrc/spotnorm.hip), the numpy f64 restatement of its
contract and an ``np.longdouble`` truth of it, shared by tests/test_spotnorm_host.py and tests/test_gpu_spotnorm.py.

The contract (get_emd.py:148-155 restated in f64; X [n, G] non-negative):
    c_i = sum_j X_ij; after = np.median(c[c > 0]); s_i = (c_i + (c_i == 0)) / after; v_ij = X_ij / s_i; l_ij = log1p(v_ij);
    m_j = sum_i l_ij / n; var_j = sum_i (l_ij - m_j)^2 / (n - 1) (two-pass); sd_j = sqrt(var_j), 0 -> 1; z_ij = (l_ij - m_j) / sd_j.
``restate`` evaluates it with numpy and scipy in a given dtype (f64: the restatement; f32: what shows that the bounds have
teeth).  ``truth`` evaluates log1p and every sum in extended precision (x86 long double: 64 bits of mantissa) without
rounding in between and rounds to f64 at the end.

The bounds (u = 2^-53; p = the ulp limit of one l against the rounded truth):
    counts, fractional data   2 (nnz_i - 1) u sum_j |X_ij|: the any-order bound of a sum, once for each side
    mean, std of column j     (n + p) 2^-52 max_i |l_ij|: (n - 1) u for a sum in any order and p ulp on each l
    z of column j             (n + 8 + p) 2^-52 (max_i |l_ij| / sd_j + max_i |z_ij|); 0 for an all-zero gene"""
import functools

import numpy as np
import scipy.sparse as sp

CHUNK = 4096                      # CS_CHUNK of csrc/colsort.h: spot counts beyond it take the median's multi-chunk path
BASE_SHAPE = (777, 301)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# restatement and truth
# ---------------------------------------------------------------------------------------------------------------------
def restate(csr, cols=None, dtype=np.float64):
    """The contract with numpy and scipy in ``dtype`` -> dict(counts, after, size_factors, L, mean, std, z); L, mean, std
    and z for the columns ``cols`` (None: all)."""
    A = sp.csr_matrix(csr).astype(dtype)
    n = A.shape[0]
    c = np.asarray(A.sum(axis=1)).ravel().astype(dtype)
    pos = c[c > 0]
    if pos.size == 0:
        raise ValueError("no spot has counts")
    after = dtype(np.median(pos))
    s = ((c + (c == 0)) / after).astype(dtype)
    dense = np.asarray(A.todense(), dtype=dtype)
    if cols is not None:
        dense = dense[:, list(cols)]
    L = np.log1p(dense / s[:, None]).astype(dtype)
    m = (L.sum(axis=0, dtype=dtype) / dtype(n)).astype(dtype)
    d = L - m
    sd = np.sqrt((d * d).sum(axis=0, dtype=dtype) / dtype(n - 1)).astype(dtype)
    sd[sd == 0] = 1
    return dict(counts=c, after=after, size_factors=s, L=L, mean=m, std=sd, z=(d / sd).astype(dtype))


def truth(csr, cols=None):
    """The contract in extended precision, rounded to f64 at the end -> the same dict."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "np.longdouble is no extended type here: the truth would be the restatement"
    X = np.asarray(sp.csr_matrix(csr).astype(np.float64).todense()).astype(ld)
    n = X.shape[0]
    c = X.sum(axis=1)
    pos = np.sort(c[c > 0])
    k = pos.size
    after = pos[k // 2] if k % 2 else (pos[k // 2 - 1] + pos[k // 2]) / ld(2)
    s = (c + (c == 0)) / after
    if cols is not None:
        X = X[:, list(cols)]
    L = np.log1p(X / s[:, None])
    assert L.dtype == ld
    m = L.sum(axis=0) / ld(n)
    d = L - m
    sd = np.sqrt((d * d).sum(axis=0) / ld(n - 1))
    sd[sd == 0] = 1
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    return dict(counts=f(c), after=float(after), size_factors=f(s), L=f(L), mean=f(m), std=f(sd), z=f(d / sd))


def ulps(got, want):
    """The largest distance of got from want in units of want's last place; a want of 0 must be met exactly (inf if not)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    zero = want == 0
    if np.any(got[zero] != 0):
        return float("inf")
    w = np.where(zero, 1.0, want)
    return float(np.max(np.where(zero, 0.0, np.abs(got - w) / np.spacing(np.abs(w)))))


def stat_bound(n, p, t):
    """Per column: the bound on mean and std against the truth dict t."""
    return (n + p) * 2.0 ** -52 * np.abs(t["L"]).max(axis=0)


def z_bound(n, p, t):
    """Per column: the bound on z against the truth dict t; exactly 0 for an all-zero gene."""
    return (n + 8 + p) * 2.0 ** -52 * (np.abs(t["L"]).max(axis=0) / t["std"] + np.abs(t["z"]).max(axis=0))


def count_bound(csr):
    """Per row: how far a sum in any order may lie from scipy's sequential one (fractional data)."""
    A = sp.csr_matrix(csr).astype(np.float64)
    nnz = np.diff(A.indptr)
    return 2.0 * np.maximum(nnz - 1, 0) * 2.0 ** -53 * np.asarray(abs(A).sum(axis=1)).ravel()


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
# what the device tests (and the ulp measurement of tools/spot_norm_rate.py) run: spots, genes, empty spots, a row with every
# gene -- 2..65 around one wave of rows, 4097 and 9001 beyond one sorted chunk (the median's multi-chunk path), an even and
# an odd number of spots with counts on both sides of it
DEVICE_SHAPES = [(2, 1, 0, False), (2, 65, 1, False), (63, 65, 1, True), (64, 301, 0, False), (65, 1, 2, False), (777, 301, 1, False),
                 (777, 301, 2, True), (4097, 65, 1, False), (4097, 301, 2, True), (9001, 301, 1, False), (9001, 1, 2, False)]
ROW_ENTRIES = (1, 64, 65, 257)        # rows 1.. of a case hold exactly so many entries where the gene count allows


@functools.lru_cache(maxsize=None)
def counts_case(n_spots, n_genes, seed=0, n_empty=1, full_row=False):
    """Poisson counts [n_spots, n_genes] (int64, dense) whose gene rates span e^-3..e^2.  Where the shape has room:
    gene 0 unexpressed, gene 1 with a single hit, gene 2 near 1000 +- 1; rows 1, 2, 3, 4 with exactly 1, 64, 65 and 257
    entries; the LAST n_empty spots empty.  full_row: no unexpressed gene, and row 5 (row 0 of a small case) holds every
    gene."""
    rs = np.random.RandomState(1000 + 7 * n_spots + 13 * n_genes + seed)
    X = rs.poisson(np.exp(rs.uniform(-3.0, 2.0, n_genes))[None, :], size=(n_spots, n_genes)).astype(np.int64)
    X[0, 0] = max(X[0, 0], 2)                                     # some spot has counts, whatever else the shape leaves
    if n_genes >= 4 and n_spots >= 8:
        X[:, 2] = 1000 + rs.randint(-1, 2, n_spots)
        X[:, 1] = 0
        X[n_spots // 2, 1] = 3
        if not full_row:
            X[:, 0] = 0
    free = np.arange(3, n_genes) if n_genes >= 4 else np.arange(n_genes)      # columns the row shaping may touch
    if n_spots >= 8:
        for r, k in enumerate(ROW_ENTRIES, start=1):
            if k > free.size:
                continue
            keep = rs.choice(free, k, replace=False)
            X[r, :] = 0
            X[r, keep] = 1 + rs.poisson(2.0, k)
    if full_row:
        r = 5 if n_spots >= 8 else 0
        X[r, :] = np.maximum(X[r, :], 1)
    if n_empty:
        X[n_spots - n_empty:, :] = 0
    return _frozen(X)


def csr_of(X, dtype=np.int32):
    m = sp.csr_matrix(np.asarray(X).astype(dtype))
    m.sum_duplicates()
    m.sort_indices()
    return m


@functools.lru_cache(maxsize=None)
def base_case():
    """777 spots x 301 genes: one empty spot, one unexpressed gene, one gene with a single hit, one near 1000 +- 1."""
    return counts_case(*BASE_SHAPE)


@functools.lru_cache(maxsize=None)
def fractional_case(n_spots=777, n_genes=301):
    """The counts of that shape times factors in [0.5, 1.5): f64 values whose sums round."""
    X = counts_case(n_spots, n_genes)
    rs = np.random.RandomState(77)
    return _frozen(X * rs.uniform(0.5, 1.5, X.shape))


@functools.lru_cache(maxsize=None)
def truth_of(n_spots, n_genes, seed=0, n_empty=1, full_row=False):
    """The truth of counts_case(...) for all genes, computed once and shared; read-only."""
    t = truth(csr_of(counts_case(n_spots, n_genes, seed, n_empty, full_row)))
    return {k: (_frozen(v) if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def nontrivial_columns(X):
    """Genes that are expressed in at least two spots: where a float32 evaluation must show."""
    return np.flatnonzero((np.asarray(X) > 0).sum(axis=0) >= 2)


# ---------------------------------------------------------------------------------------------------------------------
# .h5ad fixtures, written with the project's own h5lite in the layout of anndata 0.7+
# ---------------------------------------------------------------------------------------------------------------------
def write_h5ad(path, X, x, y, genes, layout="csr", dtype=np.float32, strings="vlen", index="_index", shuffle=None, duplicate=False,
               obs_extra=None):
    """X [n, G] dense counts -> an .h5ad at path.  layout: "csr", "csc" or "dense"; dtype: of the stored values; strings:
    "vlen" or "fixed" gene names; index: the name of var's index dataset (None: neither attribute nor dataset); shuffle: a
    RandomState that permutes the entries within every row (column) -- unsorted indices; duplicate: every entry above 1 is
    stored as two entries (1 and the rest) -- duplicates that a reader must sum."""
    from sequoia_pub_amd import h5lite
    X = np.asarray(X)
    with h5lite.File(path, "w") as f:
        if layout == "dense":
            f.create_dataset("X", data=X.astype(dtype))
        else:
            m = (sp.csr_matrix if layout == "csr" else sp.csc_matrix)(X.astype(np.float64))
            m.sort_indices()
            data, indices, indptr = m.data.copy(), m.indices.copy(), m.indptr.copy()
            if duplicate:
                extra = data > 1
                lens = np.diff(indptr)
                major = np.repeat(np.arange(len(lens)), lens)
                major = np.concatenate([major, major[extra]])
                indices = np.concatenate([indices, indices[extra]])
                data = np.concatenate([np.where(extra, 1.0, data), data[extra] - 1.0])
                order = np.argsort(major, kind="stable")
                data, indices = data[order], indices[order]
                indptr = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=len(lens)))])
            if shuffle is not None:
                for r in range(len(indptr) - 1):
                    perm = indptr[r] + shuffle.permutation(indptr[r + 1] - indptr[r])
                    data[indptr[r]:indptr[r + 1]], indices[indptr[r]:indptr[r + 1]] = data[perm], indices[perm]
            g = f.create_group("X")
            g.attrs["encoding-type"] = layout + "_matrix"
            g.attrs["encoding-version"] = "0.1.0"
            g.attrs["shape"] = np.array(X.shape, dtype=np.int64)
            g.create_dataset("data", data=data.astype(dtype))
            g.create_dataset("indices", data=indices.astype(np.int32))
            g.create_dataset("indptr", data=indptr.astype(np.int32))
        obs = f.create_group("obs")
        obs.attrs["encoding-type"] = "dataframe"
        obs.attrs["_index"] = "_index"
        obs.create_dataset("_index", data=[f"spot{i}" for i in range(X.shape[0])], string="vlen")
        obs.create_dataset("x", data=np.asarray(x))
        obs.create_dataset("y", data=np.asarray(y))
        if obs_extra is not None:
            obs_extra(f, obs)
        var = f.create_group("var")
        var.attrs["encoding-type"] = "dataframe"
        if index is not None:
            var.attrs["_index"] = index
            var.create_dataset(index, data=list(genes), string=strings)
