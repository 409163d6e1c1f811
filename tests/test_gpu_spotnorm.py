"""The device spot normalisation (sequoia_pub_amd.spotnorm, csrc/spotnorm.hip) against numpy / scipy where the contract is
exact and against the extended-precision truth of spotnorm_cases elsewhere, ``spots_from_h5ad`` and ``cli.get_emd --h5ad``.

P_DEVICE is the ulp limit of one l = log1p(x / s) against the rounded truth.  The device's own figure, measured on an
MI355X over exactly these inputs by tools/spot_norm_rate.py (profiles/spot_norm_rate.txt), is 1 ulp (largest distance
1.0 ulp, as the numpy restatement's on the CPU); the limit is that figure rounded up plus 1, and never above 8."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import gtalign_cases as gc  # noqa: E402
import spotnorm_cases as sc  # noqa: E402
from sequoia_pub_amd import _lib, gtalign, spotnorm  # noqa: E402
from sequoia_pub_amd.cli import get_emd as cli  # noqa: E402

P_DEVICE = 2
assert P_DEVICE <= 8

SHAPES = sc.DEVICE_SHAPES
COLS = {1: [0, 0, 0], 65: [64, 3, 0, 3, 17, 64, 1], 301: [300, 2, 0, 1, 2, 150, 299, 3, 2]}      # unsorted, repeated


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(gc.bits(got), gc.bits(want))


def _run(A, dtype=np.int32, **kw):
    """normalize_spots on the canonical scipy CSR A with its values as ``dtype`` -> numpy results."""
    out = spotnorm.normalize_spots(_dev(A.data.astype(dtype)), _dev(A.indices.astype(np.int32)), _dev(A.indptr.astype(np.int64)), A.shape[1], **kw)
    if isinstance(out, tuple):
        z, st = out
        assert z.is_cuda and z.dtype == torch.float64 and all(st[k].is_cuda and st[k].dtype == torch.float64 for k in ("counts", "size_factors", "mean", "std"))
        return z.cpu().numpy(), {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in st.items()}
    assert out.is_cuda and out.dtype == torch.float64
    return out.cpu().numpy()


def _exact_steps(A):
    """Steps 1-3 with numpy and scipy, as the contract words them."""
    F = A.astype(np.float64)
    c = np.asarray(F.sum(axis=1)).ravel()
    after = np.median(c[c > 0])
    return c, after, (c + (c == 0)) / after


def _check_against_truth(z, st, L, t, n, cols=None):
    """L by ulps, z, mean and std by the per-column bounds of spotnorm_cases, for the columns cols of the truth t."""
    pick = (lambda a: a) if cols is None else (lambda a: a[..., list(cols)])
    tt = {k: pick(t[k]) for k in ("L", "z", "mean", "std")}
    worst = sc.ulps(L, tt["L"])
    print(f"L: {worst:.2f} ulp from the rounded truth (limit {P_DEVICE})")
    assert worst <= P_DEVICE
    zb, sb = sc.z_bound(n, P_DEVICE, tt), sc.stat_bound(n, P_DEVICE, tt)
    ez = np.abs(z - tt["z"]).max(axis=0)
    live = zb > 0
    print(f"z: largest error / bound {float((ez[live] / zb[live]).max()) if live.any() else 0.0:.3g}")
    assert np.all(ez <= zb)                                    # an all-zero gene has bound 0: exact
    assert np.all(np.abs(st["mean"] - tt["mean"]) <= sb) and np.all(np.abs(st["std"] - tt["std"]) <= sb)
    assert np.all(z[:, ~live] == 0) and np.all(st["std"][~live] == 1.0) and np.all(st["mean"][~live] == 0)


@pytest.mark.parametrize("n_spots,n_genes,n_empty,full_row", SHAPES)
def test_integer_counts_every_shape(n_spots, n_genes, n_empty, full_row):
    _lib.require_gpu()
    X = sc.counts_case(n_spots, n_genes, 0, n_empty, full_row)
    A = sc.csr_of(X)
    entries = set(np.diff(A.indptr).tolist())
    if n_spots >= 8:                                           # the rows the kernels treat differently are there
        assert all(k in entries for k in sc.ROW_ENTRIES if k <= n_genes - 3) and (n_empty == 0 or 0 in entries) and (not full_row or n_genes in entries)
    t = sc.truth_of(n_spots, n_genes, 0, n_empty, full_row)
    z, st = _run(A, return_stats=True)
    c, after, s = _exact_steps(A)
    assert _same(st["counts"], c) and _same(np.float64(st["after"]), np.float64(after)) and _same(st["size_factors"], s)
    if n_spots >= 8 and n_genes >= 4:                          # even and odd numbers of spots with counts, on both sides of one chunk
        assert int((c > 0).sum()) == n_spots - n_empty
    L = _run(A, scale=False)
    assert z.shape == L.shape == (n_spots, n_genes)
    _check_against_truth(z, st, L, t, n_spots)
    # two calls give the same bytes
    z2, st2 = _run(A, return_stats=True)
    assert _same(z2, z) and all(_same(st2[k], st[k]) for k in ("counts", "size_factors", "mean", "std")) and st2["after"] == st["after"]
    # a column list, unsorted and repeated: the same bytes as those columns of the all-genes path
    cols = COLS[n_genes]
    zc, stc = _run(A, cols=cols, return_stats=True)
    Lc = _run(A, cols=cols, scale=False)
    assert _same(zc, z[:, cols]) and _same(Lc, L[:, cols]) and _same(stc["mean"], st["mean"][cols]) and _same(stc["std"], st["std"][cols])
    Ls, sts = _run(A, cols=cols, scale=False, return_stats=True)      # the statistics without the third pass
    assert _same(Ls, Lc) and _same(sts["mean"], stc["mean"]) and _same(sts["std"], stc["std"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_the_three_data_dtypes_agree_on_integer_counts(dtype):
    _lib.require_gpu()
    A = sc.csr_of(sc.base_case())
    z, st = _run(A, dtype=dtype, return_stats=True, cols=COLS[301])
    zi, sti = _run(A, dtype=np.int32, return_stats=True, cols=COLS[301])
    assert _same(z, zi) and all(_same(st[k], sti[k]) for k in ("counts", "size_factors", "mean", "std"))
    _check_against_truth(z, st, _run(A, dtype=dtype, scale=False, cols=COLS[301]), sc.truth_of(*sc.BASE_SHAPE), A.shape[0], COLS[301])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fractional_data(dtype):
    _lib.require_gpu()
    A = sc.csr_of(sc.fractional_case().astype(dtype), dtype)
    _, st = _run(A, dtype=dtype, return_stats=True)
    seq = np.asarray(A.astype(np.float64).sum(axis=1)).ravel()
    assert np.all(np.abs(st["counts"] - seq) <= sc.count_bound(A))
    # after and the size factors follow from the device's own counts exactly
    c = st["counts"]
    assert st["after"] == np.median(c[c > 0]) and _same(st["size_factors"], (c + (c == 0)) / st["after"])
    # L against the truth: a rounded sum of k terms is off by a relative (k - 1) u in any order, so c_i and after each move
    # s_i by that much; |dl / l| <= |dv / v| for l = log1p(v), and a relative e is at most 2 e / 2^-52 ulp
    t = sc.truth(A)
    k = int(np.diff(A.indptr).max())
    L = _run(A, dtype=dtype, scale=False)
    nz = t["L"] != 0
    worst = float(np.max(np.abs(L - t["L"])[nz] / np.spacing(np.abs(t["L"][nz]))))
    print(f"fractional L: {worst:.2f} ulp (limit {P_DEVICE + 2 * (k - 1) + 2})")
    assert np.all(L[~nz] == 0) and worst <= P_DEVICE + 2 * (k - 1) + 2


def test_refusals():
    _lib.require_gpu()
    A = sc.csr_of(sc.counts_case(40, 9, seed=3))
    data, indices, indptr = A.data.astype(np.float64), A.indices.copy(), A.indptr.astype(np.int64)
    row = int(np.flatnonzero(np.diff(indptr) >= 3)[0])
    s = indptr[row]

    def run(data=data, indices=indices, indptr=indptr, n_genes=9, **kw):
        return spotnorm.normalize_spots(_dev(data), _dev(indices), _dev(indptr), n_genes, **kw)

    swapped = indices.copy()
    swapped[s], swapped[s + 1] = indices[s + 1], indices[s]
    with pytest.raises(ValueError, match="not strictly increasing"):
        run(indices=swapped)
    twice = indices.copy()
    twice[s + 1] = indices[s]
    with pytest.raises(ValueError, match="not strictly increasing"):
        run(indices=twice)
    with pytest.raises(ValueError, match="outside"):
        run(n_genes=8)
    neg = indices.copy()
    neg[s] = -1
    with pytest.raises(ValueError, match="outside"):
        run(indices=neg)
    with pytest.raises(ValueError, match="outside"):
        run(indices=neg.astype(np.int64))
    for bad in (-1.0, np.nan, np.inf):
        d = data.copy()
        d[s + 2] = bad
        with pytest.raises(ValueError, match="negative or not finite"):
            run(data=d)
    with pytest.raises(ValueError, match="negative or not finite"):
        run(data=np.where(np.arange(len(data)) == 3, -2, A.data).astype(np.int32))
    with pytest.raises(ValueError, match="at least 2 spots"):
        run(data=data[:indptr[1]], indices=indices[:indptr[1]], indptr=indptr[:2])
    one = run(data=data[:indptr[1]], indices=indices[:indptr[1]], indptr=indptr[:2], scale=False)          # log alone takes one spot
    assert one.shape == (1, 9)
    with pytest.raises(ValueError, match="no spot has counts"):
        run(data=np.zeros_like(data))
    with pytest.raises(ValueError, match="no spot has counts"):
        run(data=data[:0], indices=indices[:0], indptr=np.zeros(41, np.int64))
    with pytest.raises(ValueError, match="indptr runs from"):
        run(indptr=indptr[1:])
    down = indptr.copy()
    assert down[4] > 0
    down[5] = down[4] - 1
    with pytest.raises(ValueError, match="indptr is not non-decreasing"):
        run(indptr=down)
    with pytest.raises(ValueError, match="column index 9 is outside"):
        run(cols=[0, 9])
    with pytest.raises(ValueError, match="dtype"):
        run(data=data.astype(np.float16))
    # over-limit sizes: the library's own message names the bound
    with pytest.raises(_lib.SequoiaHipArgError, match=f"n_genes = {spotnorm.MAX_GENES + 1}, must be in 1..{spotnorm.MAX_GENES}"):
        run(n_genes=spotnorm.MAX_GENES + 1, cols=[0])
    with pytest.raises(_lib.SequoiaHipArgError, match=f"n_spots = {spotnorm.MAX_SPOTS + 1}, must be in 1..{spotnorm.MAX_SPOTS}"):
        run(data=data[:0], indices=indices[:0], indptr=np.zeros(spotnorm.MAX_SPOTS + 2, np.int64))
    with pytest.raises(ValueError, match="does not fit 32 bits"):
        run(n_genes=2 ** 31)
    # a CPU tensor
    with pytest.raises(_lib.SequoiaHipError, match="no CPU fallback"):
        spotnorm.normalize_spots(torch.from_numpy(data), _dev(indices), _dev(indptr), 9)
    # the raw entries: a short workspace, and the arguments each refuses before any launch
    L = _lib.lib()
    stream = _lib.stream_ptr(torch.device("cuda:0"))
    counts, after, npos = torch.ones(40, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    need = int(L.sq_spot_target_workspace_bytes(40))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert need > 0 and L.sq_spot_target_workspace_bytes(0) == 0 and L.sq_spot_target_workspace_bytes(spotnorm.MAX_SPOTS + 1) == 0
    assert L.sq_spot_target(_lib.ptr(counts), 40, _lib.ptr(after), _lib.ptr(npos), _lib.ptr(ws), need - 1, stream) == -3
    assert f"workspace {need - 1} <" in L.sq_last_error().decode()
    assert L.sq_spot_target(_lib.ptr(counts), 0, _lib.ptr(after), _lib.ptr(npos), _lib.ptr(ws), need, stream) == -1 and "n_spots = 0" in L.sq_last_error().decode()
    table = torch.zeros(40, 9, dtype=torch.float64, device="cuda")
    m, sd = torch.zeros(9, dtype=torch.float64, device="cuda"), torch.zeros(9, dtype=torch.float64, device="cuda")
    for call, message in ((lambda: L.sq_spot_scale(_lib.ptr(table), 1, 9, 9, _lib.ptr(m), _lib.ptr(sd), 1, stream), "n = 1 rows"),
                          (lambda: L.sq_spot_scale(_lib.ptr(table), 40, 9, 10, _lib.ptr(m), _lib.ptr(sd), 1, stream), "C <= ld"),
                          (lambda: L.sq_spot_scale(_lib.ptr(table), 40, 9, 9, _lib.ptr(m), _lib.ptr(sd), 2, stream), "write_z = 2"),
                          (lambda: L.sq_spot_scale(None, 40, 9, 9, _lib.ptr(m), _lib.ptr(sd), 1, stream), "null")):
        assert call() == -1 and message in L.sq_last_error().decode(), (message, L.sq_last_error())
    torch.cuda.synchronize()
    assert bool((table == 0).all())                            # nothing was launched


def _write_whole_case(root):
    """The WHOLE case of gtalign_cases with raw counts in place of its expression table: stride-1.csv and spots.h5ad."""
    w = gc.whole_case()
    pred = pd.DataFrame({"xcoord": w["xcoord"], "ycoord": w["ycoord"], "xcoord_tf": w["xtf"], "ycoord_tf": w["ytf"]})
    for name, col in zip(gc.WHOLE_NAMES, w["pred"].T):
        pred[name] = col
    pred.to_csv(os.path.join(root, "stride-1.csv"), index=False)
    names = ["X5", "X6", "X7"] + gc.WHOLE_NAMES + ["X8"]          # the unexpressed, single-hit and near-1000 genes stay unrequested
    X = sc.counts_case(len(w["spot_x"]), len(names), seed=11, n_empty=1).copy()
    X[:-1, 3:8] = np.random.RandomState(12).poisson(40.0, (len(X) - 1, 5))      # the requested genes: counts rich enough that ties are rare
    sc.write_h5ad(os.path.join(root, "spots.h5ad"), X, w["spot_x"], w["spot_y"], names, layout="csr", dtype=np.float32)
    return w, X, names


def _near(values, tol):
    """Per element: how many OTHER elements lie within tol of it."""
    v = np.asarray(values, dtype=np.float64)
    return (np.abs(v[:, None] - v[None, :]) <= tol).sum(axis=1) - 1


def test_cli_h5ad_end_to_end(tmp_path):
    """``cli.get_emd --h5ad`` against ``--ground_truth`` fed with a CSV of normalize_spots' own downloaded output, and
    against ``align_ground_truth`` on ``spots_from_h5ad``.

    The second comparison is bit for bit, --emd included.  The first cannot be: --ground_truth reads its CSV with pandas'
    default float parser, as it always has, and that parser does not round-trip an f64 (measured on this machine: up to
    thousands of ulp off), so the --ground_truth run sees an expression table moved by ``moved`` -- measured here from the
    CSV itself, plus the rounding of a mean of four.  What follows from that is asserted: the prediction's columns are
    equal bit for bit; the ground truth lies within ``moved``; a median is 1-Lipschitz, so the filtered ground truth does
    too, and a percentile of score -- (left + right + (left < right)) 50 / n -- is equal bit for bit on every row with no
    other filtered value within 2 ``moved`` and within (2 k + 1) 50 / n where k others are; a distinct-value count differs
    by at most the number of rows that have such a neighbour."""
    _lib.require_gpu()
    root = str(tmp_path)
    w, X, names = _write_whole_case(root)
    genes = gc.WHOLE_GENES
    h5ad, pred_csv = os.path.join(root, "spots.h5ad"), os.path.join(root, "stride-1.csv")
    sx, sy, expr = spotnorm.spots_from_h5ad(h5ad, genes, "cuda:0")
    assert _same(sx.cpu().numpy(), w["spot_x"]) and _same(sy.cpu().numpy(), w["spot_y"]) and expr.shape == (50, 3)
    A = sc.csr_of(X)
    z = _run(A, cols=[names.index(g) for g in genes])
    assert _same(expr.cpu().numpy(), z)
    metrics_h = cli.main(["--pred_csv", pred_csv, "--h5ad", h5ad, "--out", os.path.join(root, "h"), "--gene_names", ",".join(genes)])
    truth = pd.DataFrame({"x": w["spot_x"], "y": w["spot_y"]})
    for j, g in enumerate(genes):
        truth[g] = z[:, j]
    truth.to_csv(os.path.join(root, "truth.csv"), index=False)
    metrics_c = cli.main(["--pred_csv", pred_csv, "--ground_truth", os.path.join(root, "truth.csv"), "--out", os.path.join(root, "c"),
                          "--gene_names", ",".join(genes)])
    assert sorted(os.listdir(os.path.join(root, "h"))) == sorted(os.listdir(os.path.join(root, "c"))) == ["aligned.csv", "metrics.csv"]
    parsed = pd.read_csv(os.path.join(root, "truth.csv"))[genes].values
    moved = np.abs(parsed - z).max(axis=0) + 4 * 2.0 ** -52 * np.abs(z).max(axis=0)          # per gene
    assert np.all(moved < 1e-9)
    read = lambda d, f: pd.read_csv(os.path.join(root, d, f), index_col=0, float_precision="round_trip")      # noqa: E731
    ah, ac, mh, mc = read("h", "aligned.csv"), read("c", "aligned.csv"), read("h", "metrics.csv"), read("c", "metrics.csv")
    assert list(ah.columns) == list(ac.columns) and np.array_equal(ah.index.values, ac.index.values)
    assert list(mh.columns) == list(mc.columns) == ["gene", "nr_gt_vals", "nr_gt_vals_filt"] and mh["gene"].tolist() == mc["gene"].tolist() == genes
    assert mh.values.tolist() == metrics_h.values.tolist() and mc.values.tolist() == metrics_c.values.tolist()
    col = lambda frame, c: frame[c].values.astype(np.float64)      # noqa: E731
    n = len(ah)
    for c in ("xcoord", "ycoord", "xcoord_tf", "ycoord_tf"):
        assert _same(col(ah, c), col(ac, c)), c
    for j, g in enumerate(genes):
        assert _same(col(ah, g), col(ac, g)) and _same(col(ah, g + "_filt"), col(ac, g + "_filt")), g
        gt_h, gt_c = col(ah, g + "_ground_truth"), col(ac, g + "_ground_truth")
        assert not np.isnan(gt_h).any() and not np.isnan(gt_c).any() and np.all(np.abs(gt_h - gt_c) <= moved[j]), g
        filt = gtalign.median_filter(_dev(gt_h), _dev(col(ah, "xcoord_tf")), _dev(col(ah, "ycoord_tf")), nan_absent=True).cpu().numpy()
        near = _near(filt, 2 * moved[j])
        ph, pc = col(ah, g + "_ground_truth_filt"), col(ac, g + "_ground_truth_filt")
        assert (near == 0).any() and _same(ph[near == 0], pc[near == 0]), g
        assert np.all(np.abs(ph - pc) <= (2 * near + 1) * 50.0 / n * (1 + 2.0 ** -50)), g
        assert abs(int(mh["nr_gt_vals_filt"][j]) - int(mc["nr_gt_vals_filt"][j])) <= int((near > 0).sum()), g
        assert abs(int(mh["nr_gt_vals"][j]) - int(mc["nr_gt_vals"][j])) <= int((_near(gt_h, 2 * moved[j]) > 0).sum()), g
    # the whole numeric chain from the raw file, --emd included, is align_ground_truth on spots_from_h5ad bit for bit
    cli.main(["--pred_csv", pred_csv, "--h5ad", h5ad, "--out", os.path.join(root, "e"), "--gene_names", ",".join(genes), "--emd"])
    ah, mh = read("e", "aligned.csv"), read("e", "metrics.csv")
    assert list(mh.columns) == ["gene", "emd", "nr_gt_vals", "emd_filt", "nr_gt_vals_filt"] and os.path.exists(os.path.join(root, "e", "slide_info.txt"))
    pred_back = pd.read_csv(pred_csv)
    tiles, per_gene = gtalign.align_ground_truth(_dev(pred_back[gc.WHOLE_NAMES].values.astype(np.float32)), gc.WHOLE_NAMES, _dev(w["xcoord"]),
                                                 _dev(w["ycoord"]), w["xtf"], w["ytf"], sx, sy, expr, genes, emd=True)
    assert list(ah.columns) == list(tiles.columns) and np.array_equal(ah.index.values, tiles.index.values)
    for c in tiles.columns:
        assert _same(ah[c].values.astype(np.float64), tiles[c].values.astype(np.float64)), c
    assert mh["gene"].tolist() == per_gene["gene"].tolist()
    for c in ("emd", "nr_gt_vals", "emd_filt", "nr_gt_vals_filt"):
        assert _same(mh[c].values.astype(np.float64), per_gene[c].values.astype(np.float64)), c


def test_alignment_on_the_device_table_matches_the_restatement_table(tmp_path):
    """align_ground_truth on spots_from_h5ad against align_ground_truth on the numpy restatement's z: the ground-truth
    columns -- means of four spots -- within the z bound of the columns, not by bits."""
    _lib.require_gpu()
    root = str(tmp_path)
    w, X, names = _write_whole_case(root)
    genes = gc.WHOLE_GENES
    cols = [names.index(g) for g in genes]
    sx, sy, expr = spotnorm.spots_from_h5ad(os.path.join(root, "spots.h5ad"), genes, "cuda:0")
    A = sc.csr_of(X)
    r, t = sc.restate(A, cols=cols), sc.truth(A, cols=cols)
    n = X.shape[0]
    bound = sc.z_bound(n, P_DEVICE, t) + sc.z_bound(n, 2, t)          # the device's and the restatement's distance from the truth
    assert np.all(np.abs(expr.cpu().numpy() - r["z"]).max(axis=0) <= bound)
    args = (_dev(w["pred"]), gc.WHOLE_NAMES, _dev(w["xcoord"]), _dev(w["ycoord"]), w["xtf"], w["ytf"], sx, sy)
    got, _ = gtalign.align_ground_truth(*args, expr, genes)
    want, _ = gtalign.align_ground_truth(*args, _dev(r["z"]), genes)
    assert list(got.columns) == list(want.columns) and np.array_equal(got.index.values, want.index.values)
    for j, g in enumerate(genes):
        a, b = got[g + "_ground_truth"].values, want[g + "_ground_truth"].values
        assert np.allclose(a, b, rtol=0.0, atol=bound[j] + 4 * 2.0 ** -52 * np.abs(r["z"][:, j]).max(), equal_nan=True), g
        assert _same(got[g].values, want[g].values)
