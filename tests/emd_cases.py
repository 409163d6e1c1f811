"""Seeded cases of the earth mover's distance (sequoia_pub_amd.emd, csrc/emd.hip) and what they are checked with, in plain
numpy: the grid fill, shift and normalisation of the reference's spatial_vis/get_emd.py:180-188 and calculate_emd :71-82
restated, the transportation problem solved by successive shortest augmenting paths (the device's algorithm, a dense
Dijkstra over the columns with potentials and a sparse flow), and ``check_certificate``: a feasible flow and feasible
duals of equal objective PROVE that a value is the optimum of the linear program, without trusting any solver.

The golden values (tests/golden/emd.npz, written by tests/golden/make_emd_golden.py) come from
``scipy.optimize.linprog(method="highs")``, the independent witness, each admitted only with linprog's own certificate.

Bounds of ``check_certificate`` (weights summing to 1, costs below 2^8): every quantity is the result of at most ~10^5
f64 updates of ~1e-16 each, so 1e-12 on sums of flow and 1e-10 on a dual constraint (the duals carry the costs' magnitude)
are about 10^3 above what was measured; they bound the distance from the true optimum by
gap + infeasibility + residual x max cost < 1e-9."""
import functools
import os
import zlib
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emd.npz")
COLUMN_CHUNK = 256                # sq_emd_column_chunk(): the host test holds the library to it
MAX_CELLS = 4096                  # SQ_EMD_MAX_CELLS
DEFAULT_AUGMENTATIONS = 256       # SQ_EMD_DEFAULT_AUGMENTATIONS
MARGINAL_TOL = 1e-12
DUAL_TOL = 1e-10
GAP_TOL = 1e-12
VALUE_TOL = 1e-12
GOLDEN_RTOL = 1e-9


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def fill_shift(a, b, xtf, ytf, nan_absent=True):
    """get_emd.py:180-188 for one gene: the rows present (``nan_absent``: not NaN in either column), the grid over THEIR
    extents, zeros, arr[x, y] = value, arr + abs(min(arr)).  Returns arr0 (from a), arr1 (from b)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    xtf, ytf = np.asarray(xtf).astype(np.int64), np.asarray(ytf).astype(np.int64)
    keep = ~(np.isnan(a) | np.isnan(b)) if nan_absent else np.ones(len(a), dtype=bool)
    if not keep.any():
        return np.zeros((0, 0)), np.zeros((0, 0))
    x, y = xtf[keep], ytf[keep]
    assert len(set(zip(x.tolist(), y.tolist()))) == len(x), "two rows in one grid cell"
    arr0, arr1 = np.zeros((x.max() + 1, y.max() + 1)), np.zeros((x.max() + 1, y.max() + 1))
    arr0[x, y] = a[keep]
    arr1[x, y] = b[keep]
    return arr0 + np.abs(np.min(arr0)), arr1 + np.abs(np.min(arr1))


def signature(arr):
    """calculate_emd :81-82 and cv2's skipping of zero weights: the cells with weight > 0 in row-major order ->
    (coords int64 [k, 2], weights f64 [k]); None for a grid that is all zero."""
    arr = np.asarray(arr, dtype=np.float64)
    if not np.any(arr):
        return None
    w = (arr / np.sum(arr)).ravel()
    keep = np.flatnonzero(w > 0)
    width = arr.shape[1]
    return np.stack([keep // width, keep % width], axis=1), w[keep]


def cost_matrix(ca, cb):
    d = ca[:, None, :] - cb[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float64))


class AugmentationCap(RuntimeError):
    pass


def solve(wa, ca, wb, cb, max_augmentations=None):
    """The balanced transportation problem between (wa, ca) and (wb, cb) by successive shortest augmenting paths.
    Returns value, u, v, arcs (int64 [k, 2] of (i, j), f64 [k] of flow), stats {augmentations, steps}."""
    n, m = len(wa), len(wb)
    cap = DEFAULT_AUGMENTATIONS * (n + m) if max_augmentations is None else max_augmentations
    ca, cb = np.asarray(ca, dtype=np.int64), np.asarray(cb, dtype=np.int64)

    def row_cost(i):
        dx, dy = cb[:, 0] - ca[i, 0], cb[:, 1] - ca[i, 1]
        return np.sqrt((dx * dx + dy * dy).astype(np.float64))

    u = np.zeros(n)
    v = np.full(m, np.inf)
    for i in range(n):
        v = np.minimum(v, row_cost(i))
    brem = np.array(wb, dtype=np.float64)
    flow = [OrderedDict() for _ in range(m)]                  # per column: row -> flow
    naug = steps = 0
    for s in range(n):
        supply = float(wa[s])
        while supply > 0.0 and np.any(brem > 0.0):
            if naug >= cap:
                raise AugmentationCap(f"{naug} augmentations made and supply is left")
            d = np.full(m, np.inf)
            pred = np.full(m, -1)
            fin = np.zeros(m, dtype=bool)
            dist = {s: 0.0}
            pred_col = {}
            new = [s]
            while True:
                for r in new:
                    val = (row_cost(r) - v) + (dist[r] - u[r])
                    better = ~fin & (val < d)
                    d[better] = val[better]
                    pred[better] = r
                steps += 1
                j = int(np.argmin(np.where(fin, np.inf, d)))      # the lowest index on ties
                assert not fin[j] and np.isfinite(d[j])
                fin[j] = True
                D = d[j]
                if brem[j] > 0.0:
                    break
                new = []
                for r in flow[j]:
                    if r not in dist:
                        dist[r] = D
                        pred_col[r] = j
                        new.append(r)
            v[fin] = v[fin] - (D - d[fin])
            for r, dr in dist.items():
                u[r] = u[r] + (D - dr)
            delta = min(supply, brem[j])
            path = []
            jj = j
            while True:
                r = int(pred[jj])
                path.append((r, jj))
                if r == s:
                    break
                jj = pred_col[r]
                delta = min(delta, flow[jj][r])
            for r, jj in path:
                flow[jj][r] = flow[jj].get(r, 0.0) + delta
                if r != s:
                    jb = pred_col[r]
                    f = flow[jb][r] - delta
                    if f > 0.0:
                        flow[jb][r] = f
                    else:
                        del flow[jb][r]
            supply = supply - delta
            brem[j] = brem[j] - delta
            naug += 1
    arcs = np.array([(r, j) for j in range(m) for r in flow[j]], dtype=np.int64).reshape(-1, 2)
    f = np.array([flow[j][r] for j in range(m) for r in flow[j]], dtype=np.float64)
    value = float(np.sum(f * cost_matrix(ca, cb)[arcs[:, 0], arcs[:, 1]])) if len(f) else 0.0
    return value, u, v, arcs, f, {"augmentations": naug, "steps": steps}


def emd(arr0, arr1, norm=False):
    """calculate_emd (:67-90) with the linear program's optimum where the reference calls cv2.EMD."""
    arr0, arr1 = np.asarray(arr0, dtype=np.float64), np.asarray(arr1, dtype=np.float64)
    assert arr0.shape == arr1.shape and arr0.ndim == 2
    s0, s1 = signature(arr0), signature(arr1)
    if s0 is None and s1 is None:
        return 0.0
    if s0 is None or s1 is None:
        return float("nan")
    value = solve(s0[1], s0[0], s1[1], s1[0])[0]
    return value / np.sqrt(arr0.shape[0] * arr1.shape[0]) if norm else value


def check_certificate(wa, wb, coords, u, v, arcs, value, label=""):
    """wa, wb: the weights; coords = (ca, cb) integer cell coordinates; u, v the duals; arcs = (ij int [k, 2], flow [k]).
    Asserts the five bounds of this module's docstring, prints the residuals, returns them."""
    ca, cb = coords
    ij, f = np.asarray(arcs[0]).reshape(-1, 2), np.asarray(arcs[1], dtype=np.float64)
    wa, wb, u, v = (np.asarray(t, dtype=np.float64) for t in (wa, wb, u, v))
    n, m = len(wa), len(wb)
    assert u.shape == (n,) and v.shape == (m,) and len(ij) == len(f)
    assert len(ij) == 0 or (ij.min() >= 0 and ij[:, 0].max() < n and ij[:, 1].max() < m)
    assert len(set(map(tuple, ij.tolist()))) == len(ij), "an arc is listed twice"
    c = cost_matrix(np.asarray(ca, dtype=np.int64), np.asarray(cb, dtype=np.int64))
    rows, cols = np.zeros(n), np.zeros(m)
    np.add.at(rows, ij[:, 0], f)
    np.add.at(cols, ij[:, 1], f)
    primal = float(np.sum(f * c[ij[:, 0], ij[:, 1]]))
    res = {"marginal": max(float(np.abs(rows - wa).max()), float(np.abs(cols - wb).max())),
           "min_flow": float(f.min()) if len(f) else 0.0,
           "dual_infeasibility": float((u[:, None] + v[None, :] - c).max()),
           "gap": primal - float(np.dot(u, wa) + np.dot(v, wb)),
           "value": abs(float(value) - primal), "arcs": len(f)}
    print(f"certificate {label}: n = {n}, m = {m}, arcs = {res['arcs']}, marginal {res['marginal']:.2e}, dual infeasibility "
          f"{res['dual_infeasibility']:.2e}, gap {res['gap']:.2e}, value - sum flow c {res['value']:.2e}")
    assert res["marginal"] <= MARGINAL_TOL, res
    assert res["min_flow"] >= 0.0, res
    assert res["dual_infeasibility"] <= DUAL_TOL, res
    assert res["gap"] <= GAP_TOL, res
    assert res["value"] <= VALUE_TOL, res
    return res


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def percentile(x):
    """scipy.stats.percentileofscore(x, x_i) with kind='rank' for every element (get_emd.py:21-25)."""
    x = np.asarray(x, dtype=np.float64)
    left = (x[None, :] < x[:, None]).sum(axis=1)
    right = (x[None, :] <= x[:, None]).sum(axis=1)
    return (left + right + (left < right)) * (50.0 / len(x))


def _occupied(h, w, frac, rs):
    """Rows of an h x w grid at about ``frac`` occupancy, in permuted order; the corner (h - 1, w - 1) is always there."""
    cells = [(x, y) for x in range(h) for y in range(w)]
    take = rs.permutation(len(cells) - 1)[: int(round(frac * len(cells))) - 1]
    pick = [cells[i] for i in take] + [cells[-1]]
    order = rs.permutation(len(pick))
    return np.array([pick[i][0] for i in order], dtype=np.int32), np.array([pick[i][1] for i in order], dtype=np.int32)


def _map_case(h, w, seed, kind):
    rs = np.random.RandomState(seed)
    xtf, ytf = _occupied(h, w, 0.8, rs)
    n = len(xtf)
    smooth = np.sin(xtf * 0.7) + np.cos(ytf * 0.5)
    if kind == "perc":                                       # ties from rounded values; both maps nearly one multiset
        a = percentile(np.round(smooth + 0.3 * rs.randn(n), 1))
        b = percentile(np.round(smooth + 0.3 * rs.randn(n), 1))
    else:                                                    # raw maps with negative values: every empty cell turns positive
        a = smooth + 0.5 * rs.randn(n) - 0.2
        b = (smooth + 0.5 * rs.randn(n)).astype(np.float32).astype(np.float64)
        assert a.min() < 0 and b.min() < 0
    return dict(kind="map", a=a, b=b, xtf=xtf, ytf=ytf)


def _grid(h, w, cells, rs):
    g = np.zeros((h, w))
    idx = rs.permutation(h * w)[:cells]
    g.ravel()[idx] = rs.rand(cells) + 0.05
    return g


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(kind='grid', arr0, arr1) or dict(kind='map', a, b, xtf, ytf): one problem each."""
    c = OrderedDict()
    g0, g1 = np.zeros((3, 4)), np.zeros((3, 4))
    g0[0, 1], g1[2, 3] = 2.5, 0.125
    c["single"] = dict(kind="grid", arr0=g0, arr1=g1)                                        # n = m = 1
    rs = np.random.RandomState(5)
    c["one_to_many"] = dict(kind="grid", arr0=g0.copy(), arr1=_grid(3, 4, 7, rs))            # 1 x m
    c["many_to_one"] = dict(kind="grid", arr0=_grid(3, 4, 5, rs), arr1=g1.copy())
    same = _grid(5, 6, 17, rs)
    c["identical"] = dict(kind="grid", arr0=same, arr1=same.copy())
    c["n_ne_m"] = dict(kind="grid", arr0=_grid(7, 5, 9, rs), arr1=_grid(7, 5, 23, rs))
    c["both_zero"] = dict(kind="grid", arr0=np.zeros((4, 3)), arr1=np.zeros((4, 3)))
    c["first_zero"] = dict(kind="grid", arr0=np.zeros((4, 3)), arr1=_grid(4, 3, 5, rs))
    c["second_zero"] = dict(kind="grid", arr0=_grid(4, 3, 5, rs), arr1=np.zeros((4, 3)))
    c["perc_6x7"] = _map_case(6, 7, 11, "perc")
    c["perc_12x13"] = _map_case(12, 13, 12, "perc")
    c["raw_6x7"] = _map_case(6, 7, 13, "raw")
    c["raw_12x13"] = _map_case(12, 13, 14, "raw")
    x, y = np.meshgrid(np.arange(5), np.arange(4), indexing="ij")                            # no empty cell, a positive minimum
    full = dict(kind="map", a=1.5 + rs.rand(20), b=0.25 + rs.rand(20), xtf=x.ravel().astype(np.int32), ytf=y.ravel().astype(np.int32))
    c["full_positive"] = full
    c["chunk"] = dict(kind="grid", arr0=_grid(17, 16, 37, rs), arr1=_grid(17, 16, COLUMN_CHUNK + 1, rs))
    for case in c.values():
        _frozen(*[v for v in case.values() if isinstance(v, np.ndarray)])
    return c


BATCH_SHAPE = (9, 10)
BATCH_CELLS = [(1, 1), (1, 6), (2, 2), (5, 3), (8, 8), (13, 21), (21, 13), (30, 30), (0, 0), (40, 55), (4, 0), (55, 40), (17, 64), (64, 17),
               (90, 90), (3, 77), (70, 2), (25, 26)]


@functools.lru_cache(maxsize=None)
def batch_case():
    """>= 16 problems of different sizes in one [P, H, W] pair, an all-zero pair and a one-sided zero among them."""
    rs = np.random.RandomState(21)
    h, w = BATCH_SHAPE
    arr0 = np.stack([_grid(h, w, k, rs) for k, _ in BATCH_CELLS])
    arr1 = np.stack([_grid(h, w, k, rs) for _, k in BATCH_CELLS])
    return _frozen(arr0, arr1)


TABLE_COLS_A = [4, 0, 2, 2]       # problem p compares column TABLE_COLS_A[p] of a ...
TABLE_COLS_B = [1, 3, 0, 3]       # ... with column TABLE_COLS_B[p] of b
TABLE_NAN_PROBLEM = 1             # its NaN rows are the last grid row and column: the grid shrinks


@functools.lru_cache(maxsize=None)
def table_case():
    """Two wider tables over one 6 x 7 tile grid; column 3 of b is NaN on every row of the last grid row and column."""
    rs = np.random.RandomState(31)
    xtf, ytf = _occupied(6, 7, 0.85, rs)
    n = len(xtf)
    a, b = rs.randn(n, 5), rs.randn(n, 4)
    a[:, 0] = np.abs(a[:, 0]) + 0.5
    b[(xtf == 5) | (ytf == 6), 3] = np.nan
    b[3, 3] = np.nan
    a[7, 2] = np.nan
    return _frozen(a, b, xtf, ytf)


LIMIT_SHAPE = (64, 64)            # 4096 cells, every one with weight: SQ_EMD_MAX_CELLS on both sides


@functools.lru_cache(maxsize=None)
def limit_case():
    """A pair of maps AT the cell limit that is cheap to solve: both fill a 64 x 64 grid with multiples of 1/1024 (so both
    sums are exact and equal, and untouched cells get bit-equal weights), and 12 small amounts are moved a few cells away in
    the second.  Most augmentations are one step at cost 0; the moved amounts need real searches across the whole state."""
    rs = np.random.RandomState(77)
    h, w = LIMIT_SHAPE
    arr0 = rs.randint(8, 64, size=(h, w)).astype(np.float64) / 1024.0
    arr1 = arr0.copy()
    for _ in range(12):
        px, py = rs.randint(0, h), rs.randint(0, w)
        qx, qy = np.clip(px + rs.randint(-6, 7), 0, h - 1), np.clip(py + rs.randint(-6, 7), 0, w - 1)
        if (px, py) == (qx, qy):
            continue
        amount = rs.randint(1, 8) / 1024.0
        arr1[px, py] -= amount
        arr1[qx, qy] += amount
    assert arr0.sum() == arr1.sum() and (arr1 > 0).all()
    return _frozen(arr0, arr1)


def grids_of(case):
    if case["kind"] == "grid":
        return np.asarray(case["arr0"]), np.asarray(case["arr1"])
    return fill_shift(case["a"], case["b"], case["xtf"], case["ytf"])


def case_crc(case):
    return crc(*[case[k] for k in sorted(case) if isinstance(case[k], np.ndarray)])


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: _frozen(z[k]) for k in z.files}


def close_to_golden(got, want):
    if np.isnan(want):
        return bool(np.isnan(got))
    return abs(float(got) - float(want)) <= GOLDEN_RTOL * abs(float(want))
