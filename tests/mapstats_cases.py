"""Cases of the device map statistics (sequoia_pub_amd.mapstats, csrc/mapstats.hip) and a numpy restatement of what they
compute, shared by tests/test_mapstats_host.py and tests/test_gpu_mapstats.py.

The restatement: percentile = sort, searchsorted left and right, (left + right + (left < right)) * (50.0 / n); means = a
sequential f64 sum in list order over the count; correlation = centred two-pass f64.  tests/golden/mapstats.npz holds what
the reference's literal calls give (row-by-row scipy.stats.percentileofscore, DataFrame.mean(axis=1), idxmax,
DataFrame.corr()); tests/golden/make_mapstats_golden.py makes it from the inputs defined HERE, so the inputs of the larger
cases are regenerated from their seeds (numpy's RandomState streams are frozen) and the file stays small."""
import functools
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapstats.npz")
LABELS = ("ac", "cc", "mes", "lin")
COLORS = {"ac": "#36CEBC", "cc": "#CE3649", "mes": "#3648CE", "lin": "#CEBC36"}      # gbm_celltype_analysis.py:44-47,102


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------
def percentile(values, cols=None):
    """values [n, width] (f32 or f64) -> f64 [n, C]; a column holding a NaN is all NaN (nan_policy='propagate')."""
    values = np.asarray(values)
    if values.ndim == 1:
        values = values[:, None]
    cols = range(values.shape[1]) if cols is None else cols
    n = values.shape[0]
    out = np.empty((n, len(cols)), dtype=np.float64)
    for k, c in enumerate(cols):
        a = values[:, c]
        if np.isnan(a).any():
            out[:, k] = np.nan
            continue
        s = np.sort(a)
        left, right = np.searchsorted(s, a, side="left"), np.searchsorted(s, a, side="right")
        out[:, k] = (left + right + (left < right)) * (50.0 / n)
    return out


def first_argmax(perc):
    """idxmax(axis=1) as a column number: the first largest value of each row, NaN skipped, -1 for a row of NaN."""
    perc = np.asarray(perc)
    filled = np.where(np.isnan(perc), -np.inf, perc)
    arg = filled.argmax(axis=1).astype(np.int32)
    arg[np.isnan(perc).all(axis=1)] = -1
    return arg


def category_means(pred, lists):
    """pred f32 [n, G], lists of column indices -> f64 [n, n_cat]: sequential f64 sum in list order / count; empty: NaN."""
    pred = np.asarray(pred)
    out = np.full((pred.shape[0], len(lists)), np.nan, dtype=np.float64)
    for k, members in enumerate(lists):
        if len(members) == 0:
            continue
        s = np.zeros(pred.shape[0], dtype=np.float64)
        for g in members:
            s = s + pred[:, g].astype(np.float64)
        out[:, k] = s / float(len(members))
    return out


def correlation(pred, cols=None):
    """Centred two-pass f64 Pearson matrix of the columns; a constant column gives NaN in its row and column, the diagonal
    is 1.0 elsewhere, values clipped to [-1, 1]."""
    x = np.asarray(pred)
    x = (x if cols is None else x[:, list(cols)]).astype(np.float64)
    z = x - x.mean(axis=0)
    c = z.T @ z
    sd = np.sqrt(np.diag(c))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.clip(c / (sd[:, None] * sd[None, :]), -1.0, 1.0)
    np.fill_diagonal(r, 1.0)
    const = (x == x[0]).all(axis=0)
    r[const, :] = np.nan
    r[:, const] = np.nan
    return r


# ---------------------------------------------------------------------------------------------------------------------
# percentile inputs
# ---------------------------------------------------------------------------------------------------------------------
def percentile_input(n, C, dtype, seed):
    """Multiples of 2^-10 drawn from a few values (heavy ties); column 1 (where there is one) constant; +-inf and -0.0 beside
    0.0 sprinkled over the other columns.  The same seed gives the same f32 and f64 table."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-40, 41, size=(n, C)).astype(np.float64) * 2.0 ** -10
    x += rs.randint(0, 3, size=(n, C)) * 0.25
    for c in range(C):
        if c == 1:
            x[:, c] = 0.375
            continue
        if n >= 2:
            rows = rs.choice(n, size=min(n, max(2, n // 16)), replace=False)
            special = np.array([np.inf, -np.inf, -0.0, 0.0, 0.0, -0.0, np.inf])
            x[rows, c] = special[np.arange(len(rows)) % len(special)]
    return _frozen(x.astype(dtype))


def percentile_shapes(chunk):
    return [(1, 1), (2, 3), (257, 5), (chunk - 1, 2), (chunk, 2), (chunk + 1, 3), (2 * chunk + 37, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# golden inputs (tests/golden/make_mapstats_golden.py reads these; the tests read the same)
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN_PERC = {"perc_f32": (300, 5, np.float32, 21), "perc_f64": (277, 4, np.float64, 22)}


@functools.lru_cache(maxsize=None)
def golden_percentile_input(name):
    """The tie-heavy table of percentile_input with a NaN in its last column; the f64 one is not dyadic."""
    n, C, dtype, seed = GOLDEN_PERC[name]
    x = np.array(percentile_input(n, C, dtype, seed))
    if dtype == np.float64:
        x[:, 0] = np.random.RandomState(seed + 100).randn(n) / 3.0
    x[n // 2, C - 1] = np.nan
    return _frozen(x)


DYADIC_SHAPE = (320, 40)
DYADIC_NAN_ROWS = (7, 150, 319)


@functools.lru_cache(maxsize=None)
def dyadic_table():
    """f32 [320, 40]: multiples of 2^-6 in [0, 4) drawn from a few values per gene, so that category means tie between tiles
    and percentiles tie between categories; three rows hold a NaN and are dropped.  Gene names G0..G39."""
    rs = np.random.RandomState(31)
    n, G = DYADIC_SHAPE
    x = (rs.randint(0, 5, size=(n, G)) * 0.5 + rs.randint(0, 3, size=(n, G)) * 2.0 ** -6).astype(np.float32)
    x[40:60] = x[39]                                     # identical tiles: every percentile ties
    for r in DYADIC_NAN_ROWS:
        x[r, (3 * r) % G] = np.nan
    names = [f"G{i}" for i in range(G)]
    return _frozen(x), names


def dyadic_categories():
    """Ordered label -> gene names: names absent from the table are skipped, a gene may be listed twice (cc = G1S + G2M
    share genes in the reference's lists).  3, 8, 5 and 16 genes are present: two of the divisions round."""
    return OrderedDict([("ac", ["G0", "G3", "ABSENT1", "G5"]),
                        ("cc", ["G1", "G2", "G2", "G9", "G10", "G11", "G12", "G13"]),
                        ("mes", ["G20", "ABSENT2", "G21", "G22", "G23", "G24"]),
                        ("lin", ["G30", "G31", "G32", "G33", "G34", "G35", "G36", "G37", "G38", "G39", "G4", "G6", "G7", "G14", "G15", "G16"])])


NONDYADIC_SHAPE = (300, 320)


@functools.lru_cache(maxsize=None)
def nondyadic_table():
    rs = np.random.RandomState(41)
    return _frozen((rs.rand(*NONDYADIC_SHAPE) * 6.0).astype(np.float32))


def nondyadic_lists():
    """Categories of 1, 7 and 300 genes, and an empty one (column indices)."""
    rs = np.random.RandomState(42)
    return [[17], rs.choice(320, 7, replace=False).tolist(), [], rs.permutation(320)[:300].tolist()]


CORR_SHAPES = [(2, 2), (3, 65), (33, 64), (1000, 130), (4099, 17)]
CORR_CONSTANT = {(33, 64): (5, 0.75), (1000, 130): (129, -2.5)}       # shape -> (constant column, its dyadic value)


@functools.lru_cache(maxsize=None)
def corr_input(n, K):
    """f32 [n, K]: a shared factor (so the correlations are not all near 0) on column offsets within one spread (so the
    centring matters); CORR_CONSTANT's column constant.
    Why the offsets are no larger: the bound the tests hold the device to against DataFrame.corr(), 4 n 2^-53, is the f64
    dot-product bound of the CENTRED columns, n 2^-53 a side and doubled.  pandas centres with a one-pass running-mean
    update whose error also carries a term in |mean| / spread that this bound does not include: against a long-double
    two-pass result, over 20 draws of the (3, 65) shape, DataFrame.corr() is up to 23 x 2^-53 away with offsets of +-3
    spreads and 6 x 2^-53 with offsets within one (the two-pass form: 4 in both).  Predicted expression values have
    means of the order of their spread."""
    rs = np.random.RandomState(1000 * n + K)
    x = rs.randn(n, K) + 0.7 * rs.randn(n, 1) * rs.rand(1, K) + rs.uniform(-1.0, 1.0, size=(1, K))
    x = x.astype(np.float32)
    if (n, K) in CORR_CONSTANT:
        c, v = CORR_CONSTANT[(n, K)]
        x[:, c] = v
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: _frozen(z[k]) for k in z.files}


@functools.lru_cache(maxsize=None)
def restated_correlation(n, K):
    return _frozen(correlation(corr_input(n, K)))
