"""sequoia_pub_amd.gtalign (csrc/gtalign.hip) on the device against the numpy restatement of tests/gtalign_cases.py and the
reference's literal calls in tests/golden/gtalign.npz: device == restatement == golden, compared as int64 views (every NaN
as one pattern), two calls giving the same bytes, the refusals, and the command line's two files."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import gtalign_cases as gc  # noqa: E402
from sequoia_pub_amd import _lib, gtalign  # noqa: E402
from sequoia_pub_amd.cli import get_emd as cli  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(gc.bits(got), gc.bits(want))


def _nearest(xc, yc, sx, sy, k, **kw):
    out = gtalign.nearest_spots(_dev(xc), _dev(yc), _dev(sx), _dev(sy), num_tiles=k, **kw)
    if isinstance(out, tuple):
        assert out[0].dtype == torch.int32 and out[1].dtype == torch.float64 and out[0].is_cuda and out[1].is_cuda
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    assert out.dtype == torch.int32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(gc.nearest_cases()))
def test_nearest_spots_equal_the_restatement_and_the_literal_sort(name):
    _lib.require_gpu()
    xc, yc, sx, sy, k = gc.nearest_cases()[name]
    idx, dist = _nearest(xc, yc, sx, sy, k, return_distances=True)
    want_idx, want_dist = gc.nearest(xc, yc, sx, sy, k)
    bad = int((idx != want_idx).sum()) if idx.shape == want_idx.shape else -1
    print(f"nearest {name}: {len(xc)} tiles x {len(sx)} spots, k = {k}: {bad} of {want_idx.size} indices differ")
    assert _same(idx, want_idx) and _same(idx, gc.golden()[f"ns_{name}_idx"])
    assert _same(dist, want_dist)
    again = _nearest(xc, yc, sx, sy, k)                       # without distances, and the same bytes
    assert again.tobytes() == idx.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_spot_means_equal_np_mean_of_the_kept_values(dtype):
    _lib.require_gpu()
    xc, yc, sx, sy, expr = gc.means_case(dtype)
    table = _dev(expr)
    for k in gc.MEANS_KS:
        idx = gtalign.nearest_spots(_dev(xc), _dev(yc), _dev(sx), _dev(sy), num_tiles=k)
        out = gtalign.spot_means(idx, table, cols=gc.MEANS_COLS)
        assert out.dtype == torch.float64 and out.shape == (len(xc), len(gc.MEANS_COLS)) and out.is_cuda
        got = out.cpu().numpy()
        assert _same(got, gc.spot_means(idx.cpu().numpy(), expr, gc.MEANS_COLS)), k
        assert _same(got, gc.golden()[f"means_{dtype}_k{k}"]), k
        assert gtalign.spot_means(idx, table, cols=torch.tensor(gc.MEANS_COLS, device="cuda")).cpu().numpy().tobytes() == got.tobytes()
        # no column list: a view of the first columns of the wider table (ld = 7 > C = 4)
        assert _same(gtalign.spot_means(idx, table[:, :4]).cpu().numpy(), gc.spot_means(idx.cpu().numpy(), expr[:, :4]))


@pytest.mark.parametrize("name", list(gc.median_cases()))
def test_median_filter_equals_the_restatement_and_the_literal_function(name):
    _lib.require_gpu()
    values, xtf, ytf = gc.median_cases()[name]
    v, x, y = _dev(values), _dev(xtf), _dev(ytf)
    for r in gc.MEDIAN_RADII:
        for na in (0, 1):
            out, counts = gtalign.median_filter(v, x, y, num_neighbors=r, nan_absent=bool(na), return_counts=True)
            assert out.dtype == torch.float64 and counts.dtype == torch.int32 and out.shape == values.shape
            got = out.cpu().numpy()
            want, want_counts = gc.median_filter(values, xtf, ytf, r, bool(na))
            assert _same(got, want) and _same(got, gc.golden()[f"mf_{name}_r{r}_na{na}"]), (r, na)
            assert np.array_equal(counts.cpu().numpy(), want_counts), (r, na)
            assert gtalign.median_filter(v, x, y, num_neighbors=r, nan_absent=bool(na)).cpu().numpy().tobytes() == got.tobytes()


def test_median_filter_columns_of_a_wider_table_and_a_vector():
    _lib.require_gpu()
    values, xtf, ytf = gc.median_cases()["sparse"]
    v, x, y = _dev(values), _dev(xtf), _dev(ytf)
    want = gc.golden()["mf_sparse_r1_na1"]
    assert _same(gtalign.median_filter(v, x, y, nan_absent=True, cols=[2, 0]).cpu().numpy(), want[:, [2, 0]])
    assert _same(gtalign.median_filter(v[:, :2], x, y, nan_absent=True).cpu().numpy(), want[:, :2])          # ld = 3 > C = 2
    one = gtalign.median_filter(v[:, 2].contiguous(), x.to(torch.int32), ytf, nan_absent=True)                   # ytf: a numpy array
    assert one.shape == (len(xtf),) and _same(one.cpu().numpy(), want[:, 2])
    shifted = gtalign.median_filter(v, x + 1000, y + 7, nan_absent=True)                                        # a grid that does not start at 0
    assert _same(shifted.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(gc.unique_cases()))
def test_count_unique_equals_np_unique(name):
    _lib.require_gpu()
    v = gc.unique_cases()[name]
    out = gtalign.count_unique(_dev(v))
    assert out.dtype == torch.int32 and out.shape == (1,) and out.is_cuda
    got = int(out[0])
    print(f"unique {name}: n = {len(v)}: device {got}, np.unique {int(gc.golden()[f'uq_{name}'][0])}")
    assert got == int(gc.count_unique(v)[0]) == int(gc.golden()[f"uq_{name}"][0])


def test_count_unique_of_several_columns_through_a_column_list():
    _lib.require_gpu()
    many = gc.unique_cases()["many"]
    with np.errstate(all="ignore"):
        table = np.stack([many, np.roll(many, 5) * 0.0, np.floor(many), np.full(len(many), np.nan), many * 2.0], axis=1)
    table[np.isnan(table[:, 1]), 1] = 0.0
    cols = [4, 2, 3, 1]
    with np.errstate(all="ignore"):
        want = np.array([len(np.unique(table[:, c])) for c in cols])
    t = _dev(table)
    first, again = gtalign.count_unique(t, cols=cols), gtalign.count_unique(t, cols=cols)
    assert first.cpu().numpy().tolist() == want.tolist() == gc.count_unique(table[:, cols]).tolist()
    assert first.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert gtalign.count_unique(t[:, :3]).cpu().numpy().tolist() == gc.count_unique(table[:, :3]).tolist()          # ld = 5 > C = 3


@pytest.mark.parametrize("name", ["many", "border"])
def test_count_unique_equals_the_distinct_percentiles_across_chunk_borders(name):
    """Both calls sort the same chunks with the same kernel; a value's percentile is strictly increasing in the value."""
    _lib.require_gpu()
    from sequoia_pub_amd import mapstats
    v = gc.unique_cases()[name]
    x = _dev(v[~np.isnan(v)])
    assert len(x) > gtalign.unique_chunk_rows() == mapstats.rank_chunk_rows()
    perc = mapstats.percentile_of_score(x)[:, 0].cpu().numpy()
    assert int(gtalign.count_unique(x)[0]) == len(np.unique(perc)) == len(np.unique(v[~np.isnan(v)]))


def _whole_frames():
    w = gc.whole_case()
    return gtalign.align_ground_truth(_dev(w["pred"]), gc.WHOLE_NAMES, _dev(w["xcoord"]), _dev(w["ycoord"]), w["xtf"], w["ytf"],
                                      _dev(w["spot_x"]), _dev(w["spot_y"]), _dev(w["spot_expr"]), gc.WHOLE_GENES, num_tiles=4)


def test_align_ground_truth_equals_the_literal_chain():
    _lib.require_gpu()
    g, w = gc.golden(), gc.whole_case()
    tiles, genes = _whole_frames()
    rows = np.flatnonzero(~np.isnan(w["pred"]).any(axis=1))
    assert np.array_equal(tiles.index.values, rows) and list(tiles.columns[:4]) == ["xcoord", "ycoord", "xcoord_tf", "ycoord_tf"]
    assert np.array_equal(tiles["xcoord_tf"].values, w["xtf"][rows]) and np.array_equal(tiles["ycoord"].values, w["ycoord"][rows])
    assert genes["gene"].tolist() == gc.WHOLE_GENES and list(genes.columns) == ["gene", "nr_gt_vals", "nr_gt_vals_filt"]
    for j, gene in enumerate(gc.WHOLE_GENES):
        kept = g[f"whole_{gene}_rows"]
        present = ~np.isnan(tiles[gene + "_ground_truth"].values)
        assert np.array_equal(tiles.index.values[present], kept), gene
        sub = tiles.loc[kept]
        assert _same(sub[gene + "_ground_truth"].values, g[f"whole_{gene}_ground_truth"]), gene
        assert _same(sub[gene + "_ground_truth_filt"].values, g[f"whole_{gene}_ground_truth_filt"]), gene
        assert _same(sub[gene + "_filt"].values, g[f"whole_{gene}_filt"]), gene
        assert np.array_equal(sub[gene].values, w["pred"][kept, gc.WHOLE_NAMES.index(gene)].astype(np.float64)), gene
        gone = tiles.loc[~present, [gene, gene + "_ground_truth_filt", gene + "_filt"]].values
        assert np.isnan(gone).all()
        assert [int(genes["nr_gt_vals"][j]), int(genes["nr_gt_vals_filt"][j])] == g[f"whole_{gene}_nr"].tolist(), gene
    assert int(np.isnan(tiles[gc.WHOLE_GENES[1] + "_ground_truth"].values).sum()) >= 1
    tiles2, genes2 = _whole_frames()
    pd.testing.assert_frame_equal(tiles, tiles2, check_exact=True)
    pd.testing.assert_frame_equal(genes, genes2, check_exact=True)


def test_refusals_duplicate_cells_and_out_of_range_arguments():
    _lib.require_gpu()
    x = torch.arange(6, device="cuda")
    v = torch.ones(6, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="share a grid cell"):
        gtalign.median_filter(v, torch.tensor([0, 1, 2, 1, 4, 5], device="cuda"), torch.tensor([0, 0, 0, 0, 0, 0], device="cuda"))
    with pytest.raises(ValueError, match="negative"):
        gtalign.median_filter(v, x - 1, x)
    with pytest.raises(ValueError, match="r = 4"):
        gtalign.median_filter(v, x, x, num_neighbors=4)
    with pytest.raises(ValueError, match="r = 0"):
        gtalign.median_filter(v, x, x, num_neighbors=0)
    with pytest.raises(ValueError, match="grid 4097 x 4097"):
        gtalign.median_filter(v[:2], torch.tensor([0, 4096], device="cuda"), torch.tensor([4096, 0], device="cuda"))
    with pytest.raises(ValueError, match="column index 1"):
        gtalign.median_filter(v, x, x, cols=[1])
    with pytest.raises(ValueError):
        gtalign.median_filter(v.float(), x, x)
    with pytest.raises(ValueError, match="n = 0 rows"):
        gtalign.median_filter(v[:0], x[:0], x[:0])
    c = torch.zeros(5, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="n_tiles = 0"):
        gtalign.nearest_spots(c[:0], c[:0], c, c)
    with pytest.raises(ValueError, match="n_spots = 0"):
        gtalign.nearest_spots(c, c, c[:0], c[:0])
    with pytest.raises(ValueError, match=f"n_tiles = {gtalign.MAX_ROWS + 1}"):
        big = torch.zeros(gtalign.MAX_ROWS + 1, dtype=torch.float64, device="cuda")
        gtalign.nearest_spots(big, big, c, c)
    nan = c.clone()
    nan[3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        gtalign.nearest_spots(c, c, c, nan)
    idx = torch.zeros(5, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="k_eff = 4"):
        gtalign.spot_means(idx, torch.zeros(3, 2, device="cuda"))
    with pytest.raises(ValueError, match="k_eff = 9"):
        gtalign.spot_means(torch.zeros(5, 9, dtype=torch.int32, device="cuda"), torch.zeros(30, 2, device="cuda"))
    with pytest.raises(ValueError, match="column index 2"):
        gtalign.spot_means(idx, torch.zeros(30, 2, device="cuda"), cols=[0, 2])
    with pytest.raises(ValueError, match="n = 0 rows"):
        gtalign.count_unique(c[:0])
    with pytest.raises(ValueError, match=f"n = {gtalign.MAX_ROWS + 1} rows"):
        gtalign.count_unique(torch.zeros(gtalign.MAX_ROWS + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        gtalign.count_unique(c.cpu())
    # a spot index outside the table is not followed: that mean is NaN, its neighbours are computed
    idx[2, 1] = 30
    idx[3, 0] = -1
    out = gtalign.spot_means(idx, torch.ones(30, 2, device="cuda")).cpu().numpy()
    assert np.isnan(out[[2, 3]]).all() and np.all(out[[0, 1, 4]] == 1.0)


def test_non_default_stream_and_the_largest_counts():
    _lib.require_gpu()
    xc, yc, sx, sy, k = gc.nearest_cases()["chunk_4099"]
    args = [_dev(a) for a in (xc, yc, sx, sy)]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        idx = gtalign.nearest_spots(*args, num_tiles=k).cpu().numpy()
    assert _same(idx, gc.golden()["ns_chunk_4099_idx"])
    # SQ_MAP_MAX_ROWS rows of one column: 64 chunks, every chunk holding every value
    big = (np.random.RandomState(91).randint(0, 777, gtalign.MAX_ROWS) * 0.25)
    assert int(gtalign.count_unique(_dev(big))[0]) == 777


def test_cli_writes_metrics_and_aligned(tmp_path):
    _lib.require_gpu()
    w = gc.whole_case()
    root = str(tmp_path)
    pred = pd.DataFrame({"xcoord": w["xcoord"], "ycoord": w["ycoord"], "xcoord_tf": w["xtf"], "ycoord_tf": w["ytf"]})
    for name, col in zip(gc.WHOLE_NAMES, w["pred"].T):
        pred[name] = col
    pred.to_csv(os.path.join(root, "stride-1.csv"), index=False)
    truth = pd.DataFrame({"x": w["spot_x"], "y": w["spot_y"]})
    for j, gene in enumerate(gc.WHOLE_GENES):
        truth[gene] = w["spot_expr"][:, j]
    truth["unused"] = 1.0
    truth.to_csv(os.path.join(root, "truth.csv"), index=False)
    out = os.path.join(root, "out")
    metrics = cli.main(["--pred_csv", os.path.join(root, "stride-1.csv"), "--ground_truth", os.path.join(root, "truth.csv"), "--out", out,
                        "--gene_names", ",".join(gc.WHOLE_GENES)])
    # what the command line reads back: the f32 predictions exactly, the expression as the f64 the CSV parser gives
    pred_back, truth_back = pd.read_csv(os.path.join(root, "stride-1.csv")), pd.read_csv(os.path.join(root, "truth.csv"))
    assert np.array_equal(pred_back[gc.WHOLE_NAMES].values.astype(np.float32), w["pred"], equal_nan=True)
    tiles, genes = gtalign.align_ground_truth(_dev(pred_back[gc.WHOLE_NAMES].values.astype(np.float32)), gc.WHOLE_NAMES, _dev(w["xcoord"]),
                                              _dev(w["ycoord"]), w["xtf"], w["ytf"], _dev(w["spot_x"]), _dev(w["spot_y"]),
                                              _dev(truth_back[gc.WHOLE_GENES].values), gc.WHOLE_GENES)
    got = pd.read_csv(os.path.join(out, "metrics.csv"), index_col=0)
    assert list(got.columns) == ["gene", "nr_gt_vals", "nr_gt_vals_filt"] and got.values.tolist() == genes.values.tolist() == metrics.values.tolist()
    aligned = pd.read_csv(os.path.join(out, "aligned.csv"), index_col=0, float_precision="round_trip")
    assert list(aligned.columns) == list(tiles.columns) and np.array_equal(aligned.index.values, tiles.index.values)
    for c in tiles.columns:
        assert _same(aligned[c].values.astype(np.float64), tiles[c].values.astype(np.float64)), c
