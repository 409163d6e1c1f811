"""Cases of the device ground-truth alignment (sequoia_pub_amd.gtalign, csrc/gtalign.hip) and a numpy restatement of what
it computes, shared by tests/test_gtalign_host.py and tests/test_gpu_gtalign.py.

The restatement:
    nearest spots   d = sqrt(dx dx + dy dy) in f64, every operation rounded on its own; the first k of a STABLE sort by d.
    means           numpy's sum of the k kept values over k: ((0.0 + e0) + e1) + ... for k <= 7 and, for k = 8, numpy's
                    unrolled pairwise block 0.0 + (((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7))).
    median filter   a window of c rows; 2 c > (2 r + 1)^2: NaN if a member is NaN, 0.0 + the middle value (odd c) or
                    ((0.0 + a) + b) / 2.0 (even c) -- np.median ends in np.mean, which starts its sum at 0.0, so a median
                    of -0.0 is 0.0 -- otherwise the row's own value.
    unique          -0.0 and 0.0 one value, all NaNs together one.
tests/golden/gtalign.npz holds what the reference's literal get_average, median_filter, score2percentile and np.unique
give; tests/golden/make_gtalign_golden.py makes it from the inputs defined HERE, which are regenerated from their seeds
(numpy's RandomState streams are frozen), so the file stays small.  NaN results are compared as NaN: the sign and payload
of a NaN (x86 gives -nan for inf - inf) are not part of the contract."""
import functools
import os
from collections import OrderedDict
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtalign.npz")
SPOT_CHUNK = 2048                 # sq_gt_spot_chunk(): the host test holds the library to it
UNIQUE_CHUNK = 4096               # sq_gt_unique_chunk_rows()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def bits(a):
    """f64 -> int64 views with every NaN mapped to one pattern; other dtypes unchanged."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a
    v = a.view(np.int64).copy()
    v[np.isnan(a)] = np.int64(0x7FF8000000000000)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------
def distances(xc, yc, sx, sy):
    dx = np.asarray(sx, dtype=np.float64)[None, :] - np.asarray(xc, dtype=np.float64)[:, None]
    dy = np.asarray(sy, dtype=np.float64)[None, :] - np.asarray(yc, dtype=np.float64)[:, None]
    return np.sqrt(dx * dx + dy * dy)


def nearest(xc, yc, sx, sy, k):
    """-> (int32 [n_tiles, k_eff], f64 [n_tiles, k_eff]), k_eff = min(k, n_spots)."""
    d = distances(xc, yc, sx, sy)
    k_eff = min(k, d.shape[1])
    idx = np.argsort(d, axis=1, kind="stable")[:, :k_eff]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=1)


def spot_means(idx, expr, cols=None):
    expr = np.asarray(expr)
    e = (expr if cols is None else expr[:, list(cols)]).astype(np.float64)
    k = idx.shape[1]
    v = [e[idx[:, j]] for j in range(k)]                                  # k arrays [n_tiles, C]
    with np.errstate(all="ignore"):                                       # inf + -inf is a case
        if k == 8:
            s = 0.0 + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
        else:
            s = np.zeros_like(v[0])
            for j in range(k):
                s = s + v[j]
        return s / float(k)


def median_filter(values, xtf, ytf, r, nan_absent):
    """values f64 [n, C] -> (f64 [n, C], int32 [n, C] window counts)."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        values = values[:, None]
    xtf, ytf = np.asarray(xtf), np.asarray(ytf)
    n, C = values.shape
    out = np.empty((n, C), dtype=np.float64)
    counts = np.empty((n, C), dtype=np.int32)
    full = (2 * r + 1) ** 2
    with np.errstate(all="ignore"):
        for i in range(n):
            near = (np.abs(xtf - xtf[i]) <= r) & (np.abs(ytf - ytf[i]) <= r)
            for c in range(C):
                w = values[near, c]
                if nan_absent:
                    w = w[~np.isnan(w)]
                counts[i, c] = len(w)
                own = values[i, c]
                if nan_absent and np.isnan(own):
                    out[i, c] = np.nan
                elif 2 * len(w) > full:
                    if np.isnan(w).any():
                        out[i, c] = np.nan
                    else:
                        s = np.sort(w)
                        m = len(s) // 2
                        out[i, c] = 0.0 + s[m] if len(s) % 2 else ((0.0 + s[m - 1]) + s[m]) / 2.0
                else:
                    out[i, c] = own
    return out, counts


def count_unique(values):
    """f64 [n, C] (or [n]) -> int32 [C]."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        values = values[:, None]
    out = np.zeros(values.shape[1], dtype=np.int32)
    for c in range(values.shape[1]):
        v = values[:, c]
        nan = np.isnan(v)
        s = np.sort(v[~nan])
        out[c] = (1 if len(s) else 0) + int((s[1:] != s[:-1]).sum()) + int(nan.any())
    return out


def percentile(a):
    """scipy.stats.percentileofscore(a, x) for every x of the vector a (kind='rank'); a NaN anywhere: all NaN."""
    a = np.asarray(a, dtype=np.float64)
    if np.isnan(a).any():
        return np.full(len(a), np.nan)
    s = np.sort(a)
    left, right = np.searchsorted(s, a, side="left"), np.searchsorted(s, a, side="right")
    return (left + right + (left < right)) * (50.0 / len(a))


# ---------------------------------------------------------------------------------------------------------------------
# nearest-spot cases: name -> (xc, yc, sx, sy, k)
# ---------------------------------------------------------------------------------------------------------------------
LATTICE_INTERIOR = [5 * i + j for i in (1, 2, 3) for j in (1, 2, 3)]      # tiles whose 4 x 4 block of lattice points is whole


def _lattice():
    """36 points of a 6 x 6 lattice of pitch 100 and one more beside it, in permuted index order; tiles at the 25 cell
    centres.  An interior tile has 4 spots at 50 sqrt 2 and 8 at sqrt(150^2 + 50^2), each ring an exact tie."""
    rs = np.random.RandomState(101)
    pts = [(100.0 * i, 100.0 * j) for i in range(6) for j in range(6)] + [(600.0, 0.0)]
    pts = np.array(pts)[rs.permutation(37)]
    cx, cy = np.meshgrid(np.arange(5) * 100.0 + 50.0, np.arange(5) * 100.0 + 50.0, indexing="ij")
    return cx.ravel().copy(), cy.ravel().copy(), pts[:, 0].copy(), pts[:, 1].copy()


@functools.lru_cache(maxsize=None)
def sqrt_collapse_pair(k=4):
    """A seeded search over float coordinates: a tile and two spots whose d^2 are one ulp apart and whose d are equal, the
    LARGER d^2 at index 0 and the smaller at index 1; k - 1 closer spots behind them and farther ones behind those.  A
    stable sort by d keeps the closer ones and index 0; a sort by d^2 keeps index 1 instead."""
    rs = np.random.RandomState(202)
    for attempt in range(1_000_000):
        tx, ty = rs.uniform(-1.0, 1.0, 2)                        # small, so that one ulp of a spot coordinate is about one of dx
        ax, ay = tx + rs.uniform(100.0, 200.0), ty + rs.uniform(100.0, 200.0)
        bx = np.nextafter(ax, np.inf)
        d2a = (ax - tx) * (ax - tx) + (ay - ty) * (ay - ty)
        d2b = (bx - tx) * (bx - tx) + (ay - ty) * (ay - ty)
        if d2b == np.nextafter(d2a, np.inf) and np.sqrt(d2a) == np.sqrt(d2b):
            break
    else:
        raise AssertionError("no sqrt-collapse pair in 10^6 candidates")
    ang = rs.uniform(0.0, 2.0 * np.pi, k - 1 + 6)
    rad = np.concatenate([rs.uniform(20.0, 90.0, k - 1), rs.uniform(400.0, 900.0, 6)])
    sx = np.concatenate([[bx, ax], tx + rad * np.cos(ang)])
    sy = np.concatenate([[ay, ay], ty + rad * np.sin(ang)])
    return _frozen(np.array([tx]), np.array([ty]), sx, sy) + (k, attempt)


def fma_d2(dx, dy):
    """fma(dx, dx, fl(dy dy)): the product dx dx exact, one rounding -- what a contracted dx*dx + dy*dy computes."""
    return float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy))


@functools.lru_cache(maxsize=None)
def contraction_pair():
    """A seeded search: a tile and the spots A = tile + (p, q), B = tile + (q, p), whose separately rounded d^2 are EQUAL
    (the sum commutes) so that the lower index wins, while fma(dx, dx, dy dy) gives them different d^2 AND different d.
    The fused form comes in two shapes, fma(dx, dx, dy dy) and fma(dy, dy, dx dx), and they swap the roles of A and B: the
    case is used with the spots in both orders, so whichever shape a compiler picks, one order keeps the wrong spot.
    Tile coordinates are multiples of 1024 and p, q carry 30 bits, so tile + p - tile is p exactly."""
    rs = np.random.RandomState(303)
    tx, ty = 1024.0, 2048.0
    for attempt in range(1_000_000):
        p = float(rs.randint(1 << 29, 1 << 30)) * 2.0 ** -22
        q = float(rs.randint(1 << 29, 1 << 30)) * 2.0 ** -22
        u, v = fma_d2(p, q), fma_d2(q, p)
        if u != v and np.sqrt(u) != np.sqrt(v) and (tx + p) - tx == p and (ty + q) - ty == q and (tx + q) - tx == q and (ty + p) - ty == p:
            return tx, ty, p, q, attempt
    raise AssertionError("no contraction case in 10^6 candidates")


def chunk_near_indices(n_spots):
    """Where the true neighbours sit: the last two spots (the last, partial, chunk) and both sides of the last chunk border."""
    last_start = (n_spots - 1) // SPOT_CHUNK * SPOT_CHUNK
    return sorted({n_spots - 1, max(n_spots - 2, 0), last_start, max(last_start - 1, 0)})


def _chunk_case(n_spots, seed):
    rs = np.random.RandomState(seed)
    sx, sy = rs.uniform(0.0, 10000.0, n_spots), rs.uniform(0.0, 10000.0, n_spots)
    keep_off = np.hypot(sx - 5000.0, sy - 5000.0) < 400.0                 # nothing random near the tiles
    sx[keep_off] += 1000.0
    near = chunk_near_indices(n_spots)
    for r, i in enumerate(near):
        sx[i], sy[i] = 5000.0 + 7.0 * (r + 1) * (-1) ** r, 5000.0 + 3.0 * (r + 1)
    xc = 5000.0 + rs.uniform(-5.0, 5.0, 5)
    yc = 5000.0 + rs.uniform(-5.0, 5.0, 5)
    return xc, yc, sx, sy


def _random_case(n_tiles, n_spots, seed, centre=0.0, spread=1000.0):
    rs = np.random.RandomState(seed)
    return (centre + rs.uniform(-spread, spread, n_tiles), centre + rs.uniform(-spread, spread, n_tiles),
            centre + rs.uniform(-spread, spread, n_spots), centre + rs.uniform(-spread, spread, n_spots))


@functools.lru_cache(maxsize=None)
def nearest_cases():
    cases = OrderedDict()
    for k in (1, 4, 8):
        cases[f"ties_k{k}"] = _lattice() + (k,)
    cases["sqrt_collapse"] = sqrt_collapse_pair()[:5]
    tx, ty, p, q, _ = contraction_pair()
    far = ([tx + 5.0 * p, tx - 4.0 * p], [ty + 3.0 * q, ty - 6.0 * q])
    cases["contraction_ab"] = (np.array([tx]), np.array([ty]), np.array([tx + p, tx + q] + far[0]), np.array([ty + q, ty + p] + far[1]), 1)
    cases["contraction_ba"] = (np.array([tx]), np.array([ty]), np.array([tx + q, tx + p] + far[0]), np.array([ty + p, ty + q] + far[1]), 1)
    cases["spots_1"] = _random_case(7, 1, 401) + (4,)
    cases["spots_3"] = _random_case(7, 3, 402) + (4,)
    cases["spots_eq_k"] = _random_case(7, 4, 403) + (4,)
    for n_spots in (SPOT_CHUNK - 1, SPOT_CHUNK, SPOT_CHUNK + 1, 2 * SPOT_CHUNK + 3):
        cases[f"chunk_{n_spots}"] = _chunk_case(n_spots, 410 + n_spots % 7) + (4,)
    for n_tiles in (1, 63, 65, 257):
        cases[f"tiles_{n_tiles}"] = _random_case(n_tiles, 50, 420 + n_tiles) + (4,)
    cases["near_1e5"] = _random_case(40, 90, 431, centre=1.0e5, spread=300.0) + (4,)
    cases["negative"] = _random_case(40, 90, 432, centre=-150.0, spread=400.0) + (5,)
    cases["slide"] = _random_case(300, 5000, 433, centre=20000.0, spread=15000.0) + (4,)
    for c in cases.values():
        _frozen(*[a for a in c[:4]])
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# means cases
# ---------------------------------------------------------------------------------------------------------------------
MEANS_COLS = [5, 0, 3]                 # a permuted subset of a table with ld = 7
MEANS_KS = (3, 4, 7, 8)
MEANS_SHAPE = (60, 50)                 # tiles, spots


@functools.lru_cache(maxsize=None)
def means_case(dtype_name):
    """60 tiles, 50 spots; expression spread over seven decades so that the order of the adds shows; a NaN and an
    infinity in spots that tile 0 keeps (k = 3), a row of -0.0.  -> (xc, yc, sx, sy, expr [50, 7])."""
    xc, yc, sx, sy = _random_case(MEANS_SHAPE[0], MEANS_SHAPE[1], 501)
    rs = np.random.RandomState(502)
    expr = rs.randn(MEANS_SHAPE[1], 7) * 10.0 ** rs.randint(-3, 4, size=(MEANS_SHAPE[1], 7))
    first = nearest(xc[:1], yc[:1], sx, sy, 3)[0][0]
    expr[first[0], 5] = np.nan
    expr[first[1], 0] = np.inf
    expr[first[2], 0] = -np.inf                                   # inf + -inf in column 0 of tile 0
    last = nearest(xc[-1:], yc[-1:], sx, sy, 8)[0][0]
    if not set(last) & set(first):
        expr[last, 3] = -0.0                                       # a mean of eight -0.0 is 0.0
    return _frozen(xc, yc, sx, sy, expr.astype(np.dtype(dtype_name)))


# ---------------------------------------------------------------------------------------------------------------------
# median-filter cases: name -> (values [n, C], xtf, ytf); every case runs with r = 1, 2, 3 and nan_absent = 0, 1
# ---------------------------------------------------------------------------------------------------------------------
def _grid_rows(occupied, rs):
    """The occupied cells of a boolean [w, h] array as rows in PERMUTED order."""
    x, y = np.nonzero(occupied)
    order = rs.permutation(len(x))
    return x[order].astype(np.int64), y[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def median_cases():
    cases = OrderedDict()
    rs = np.random.RandomState(601)
    # a sparse 13 x 11 grid whose occupancy rises from 0.3 to 0.95 along x: windows of every count up to the full one
    prob = np.linspace(0.3, 0.95, 13)[:, None]
    x, y = _grid_rows(rs.rand(13, 11) < prob, rs)
    v = np.round(rs.randn(len(x), 3) * 4.0, 1)                     # one decimal: ties between tiles
    v[rs.choice(len(x), 5, replace=False), 0] = np.nan            # three columns with different NaN rows
    v[rs.choice(len(x), 3, replace=False), 1] = np.nan
    cases["sparse"] = (v, x, y)
    x, y = _grid_rows(np.ones((5, 4), dtype=bool), rs)            # corners (4 rows at r = 1), edges (6), interior (9)
    cases["full"] = (rs.randn(20, 1) * 3.0, x, y)
    cases["one"] = (np.array([[2.5]]), np.array([0]), np.array([0]))
    cases["line"] = (rs.randn(7, 1), np.zeros(7, dtype=np.int64), rs.permutation(7).astype(np.int64))
    # 3 x 2 full grids: the two rows of the middle column see all 6 rows (even: the mean of the two middle values)
    x6, y6 = np.array([0, 0, 1, 1, 2, 2]), np.array([0, 1, 0, 1, 0, 1])
    big = 1.7e308
    six = OrderedDict([("zeros", [-1.0, -2.0, -0.0, 0.0, 3.0, 4.0]), ("neg_zeros", [-1.0, -2.0, -0.0, -0.0, 3.0, 4.0]),
                       ("inf_inf", [1.0, 2.0, 3.0, np.inf, np.inf, np.inf]), ("minf_inf", [-np.inf, -np.inf, -np.inf, np.inf, np.inf, np.inf]),
                       ("overflow", [1.0, 2.0, big, big, 1.75e308, 1.79e308]), ("nan", [1.0, 2.0, np.nan, 4.0, 5.0, 6.0])])
    for name, vals in six.items():
        order = rs.permutation(6)
        cases["six_" + name] = (np.array(vals)[order][:, None], x6[order], y6[order])
    x9, y9 = _grid_rows(np.ones((3, 3), dtype=bool), rs)          # an odd count whose middle value is -0.0
    cases["nine_neg_zero"] = (np.array([-3.0, -2.0, -1.0, -0.0, -0.0, -0.0, 1.0, 2.0, 3.0])[rs.permutation(9)][:, None], x9, y9)
    for c in cases.values():
        _frozen(*c)
    return cases


MEDIAN_RADII = (1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# unique cases: name -> f64 [n]
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unique_cases():
    rs = np.random.RandomState(701)
    cases = OrderedDict()
    cases["one"] = np.array([3.25])
    cases["equal"] = np.full(300, -1.5)
    cases["distinct"] = rs.permutation(1000).astype(np.float64) * 0.37
    cases["specials"] = np.array([0.0, -0.0, np.nan, np.nan, 1.0])
    border = rs.randint(0, 40, UNIQUE_CHUNK + 50).astype(np.float64) * 0.5        # every value on both sides of the border
    border[UNIQUE_CHUNK - 1], border[UNIQUE_CHUNK] = 1234.5, 1234.5
    cases["border"] = border
    many = rs.randint(0, 3000, 2 * UNIQUE_CHUNK + 37).astype(np.float64) * 2.0 ** -3
    many[rs.choice(len(many), 9, replace=False)] = [np.nan, np.nan, np.inf, np.inf, -np.inf, -0.0, 0.0, -0.0, np.nan]
    cases["many"] = many
    cases["all_nan"] = np.full(17, np.nan)
    for c in cases.values():
        _frozen(c)
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the whole function
# ---------------------------------------------------------------------------------------------------------------------
WHOLE_GENES = ["G2", "G0", "G3"]       # requested, in this order; the table has five
WHOLE_NAMES = ["G0", "G1", "G2", "G3", "G4"]
WHOLE_NAN_ROW = 17                     # a tile whose prediction holds a NaN: dropped first


@functools.lru_cache(maxsize=None)
def whole_case():
    """Sixty tiles on a full 10 x 6 grid of pitch 224 (rows permuted), fifty spots, three genes out of five predicted; the
    expression of WHOLE_GENES[1] is NaN in a spot that some tile keeps, so that gene loses rows of its own.
    -> dict(pred f32 [60, 5], xcoord, ycoord, xtf, ytf, spot_x, spot_y, spot_expr f32 [50, 3])."""
    rs = np.random.RandomState(801)
    order = rs.permutation(60)
    xtf, ytf = (np.arange(60) // 6)[order], (np.arange(60) % 6)[order]
    xcoord, ycoord = 3000.0 + 224.0 * xtf, 1000.0 + 224.0 * ytf
    spot_x = 3000.0 + rs.uniform(-100.0, 2300.0, 50)
    spot_y = 1000.0 + rs.uniform(-100.0, 1400.0, 50)
    spot_expr = np.round(rs.randn(50, 3), 1).astype(np.float32)                 # one decimal: ties between tiles
    kept = nearest(xcoord[5:6], ycoord[5:6], spot_x, spot_y, 4)[0][0]
    spot_expr[kept[2], 1] = np.nan
    pred = np.round(rs.rand(60, 5) * 4.0, 1).astype(np.float32)
    pred[WHOLE_NAN_ROW, 4] = np.nan
    out = dict(pred=pred, xcoord=xcoord, ycoord=ycoord, xtf=xtf.astype(np.int64), ytf=ytf.astype(np.int64), spot_x=spot_x, spot_y=spot_y,
               spot_expr=spot_expr)
    _frozen(*out.values())
    return out


def whole_restated():
    """The chain of get_emd.py:164-175 and :204-205 on whole_case() through the restatement.
    -> rows, {gene: dict(sub, ground_truth, ground_truth_filt, pred_filt, nr_gt_vals, nr_gt_vals_filt)}."""
    w = whole_case()
    rows = np.flatnonzero(~np.isnan(w["pred"]).any(axis=1))
    idx, _ = nearest(w["xcoord"][rows], w["ycoord"][rows], w["spot_x"], w["spot_y"], 4)
    gt = spot_means(idx, w["spot_expr"])
    filt, _ = median_filter(gt, w["xtf"][rows], w["ytf"][rows], 1, True)
    out = OrderedDict()
    for j, g in enumerate(WHOLE_GENES):
        sub = np.flatnonzero(~np.isnan(gt[:, j]))
        pf = percentile(filt[sub, j])
        out[g] = dict(sub=sub, ground_truth=gt[sub, j], ground_truth_filt=pf,
                      pred_filt=percentile(w["pred"][rows][sub, WHOLE_NAMES.index(g)].astype(np.float64)),
                      nr_gt_vals=int(count_unique(gt[sub, j])[0]), nr_gt_vals_filt=int(count_unique(pf)[0]))
    return rows, out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: _frozen(z[k]) for k in z.files}
