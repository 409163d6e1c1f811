"""sequoia_pub_amd.mapstats (csrc/mapstats.hip) on the device against the numpy restatement of tests/mapstats_cases.py and
the reference's literal calls in tests/golden/mapstats.npz: percentiles bit-equal to scipy's, category means bit-equal to
pandas on dyadic tables and within the f64 summation bound otherwise, the cell-type frame of the dyadic golden equal in
every mean, percentile, label and colour, the gene correlation within the f64 dot-product bound of DataFrame.corr(), the
refusals, and the command line's three kinds of CSV."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import mapstats_cases as mc  # noqa: E402
from sequoia_pub_amd import _lib, mapstats  # noqa: E402
from sequoia_pub_amd.cli import gbm_celltype_analysis as cli  # noqa: E402

U = 2.0 ** -53


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _percentile(x, **kw):
    out = mapstats.percentile_of_score(_dev(x) if not torch.is_tensor(x) else x, **kw)
    first = None
    if isinstance(out, tuple):
        out, first = out
        assert first.dtype == torch.int32 and first.is_cuda
    assert out.dtype == torch.float64 and out.is_cuda
    return (out.cpu().numpy(), first.cpu().numpy()) if first is not None else out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_percentile_shapes_are_bit_equal_to_the_restatement(dtype):
    _lib.require_gpu()
    c = mapstats.rank_chunk_rows()
    for k, (n, C) in enumerate(mc.percentile_shapes(c)):
        x = mc.percentile_input(n, C, dtype, 50 + k)
        got, want = _percentile(x), mc.percentile(x)
        bad = int((got != want).sum())
        print(f"percentile {np.dtype(dtype).name} n={n} C={C}: {bad} of {got.size} differ; distinct values {len(np.unique(want))}")
        assert got.shape == (n, C) and np.array_equal(got, want), (n, C, np.argwhere(got != want)[:5].tolist())
        if n > 1 and C > 1:
            assert len(np.unique(got[:, 1])) == 1 and got[0, 1] == (n + 1) * (50.0 / n)             # the constant column


def test_percentile_cols_gather_with_a_wider_table_and_a_repeated_column():
    _lib.require_gpu()
    c = mapstats.rank_chunk_rows()
    for dtype in (np.float32, np.float64):
        x = mc.percentile_input(c + 5, 9, dtype, 71)
        cols = [7, 0, 7, 3]
        got = _percentile(x, cols=cols)
        assert np.array_equal(got, mc.percentile(x, cols)) and np.array_equal(got[:, 0], got[:, 2])
        # a view of the first columns of a wider table: ld > C with no column list; and a device column list
        wide = _dev(x)
        assert np.array_equal(_percentile(wide[:, :4]), mc.percentile(x[:, :4]))
        assert np.array_equal(_percentile(wide, cols=torch.tensor(cols, device="cuda")), got)
        assert np.array_equal(_percentile(wide[:, 2]), mc.percentile(x[:, 2]))                          # one column, stride 9


def test_a_nan_makes_its_column_nan_and_leaves_the_others():
    _lib.require_gpu()
    c = mapstats.rank_chunk_rows()
    for dtype in (np.float32, np.float64):
        x = np.array(mc.percentile_input(c + 300, 4, dtype, 72))
        clean = mc.percentile(x)
        x[c + 17, 2] = np.nan                                       # in the second chunk
        x[5, 0] = np.nan
        got, first = _percentile(x, return_argmax=True)
        assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 2]).all()
        assert np.array_equal(got[:, [1, 3]], clean[:, [1, 3]])
        assert np.array_equal(first, mc.first_argmax(got)) and set(first.tolist()) <= {1, 3}


def test_argmax_takes_the_first_of_tied_maxima_and_minus_one_for_a_row_of_nan():
    _lib.require_gpu()
    # columns 1 and 3 equal, column 2 their negative: rows where 1 and 3 tie for the lead, and rows led by 2
    rs = np.random.RandomState(73)
    base = (rs.randint(0, 50, 600) * 0.125).astype(np.float32)
    x = np.stack([base * 0 + 1.0, base, -base, base], axis=1)
    got, first = _percentile(x, return_argmax=True)
    want = mc.percentile(x)
    assert np.array_equal(got, want) and np.array_equal(first, mc.first_argmax(want))
    assert int((first == 1).sum()) > 50 and int((first == 2).sum()) > 50 and int((first == 3).sum()) == 0
    assert bool((got[:, 1] == got[:, 3]).all()) and int(((first == 1) & (got[:, 1] > got[:, 0])).sum()) > 50
    allnan = np.full((5, 3), np.nan, dtype=np.float64)
    allnan[2, 1] = 1.0                                              # one number: its column is NaN all the same
    got, first = _percentile(allnan, return_argmax=True)
    assert np.isnan(got).all() and first.tolist() == [-1] * 5


@pytest.mark.parametrize("name", list(mc.GOLDEN_PERC))
def test_percentile_is_bit_equal_to_scipy_on_the_golden(name):
    _lib.require_gpu()
    want = mc.golden()[name + "_out"]
    got = _percentile(mc.golden_percentile_input(name))
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))


def test_means_are_bit_equal_to_pandas_on_dyadic_tables():
    _lib.require_gpu()
    g = mc.golden()
    x, names = mc.dyadic_table()
    rows = g["dyadic_rows"]
    lists = mapstats.category_indices(names, mc.dyadic_categories())
    got = mapstats.category_means(_dev(x[rows]), lists).cpu().numpy()
    assert np.array_equal(got, g["dyadic_means"])
    # categories of 1, 7 and 300 genes and an empty one on a dyadic table: every sum exact, one rounded division
    rs = np.random.RandomState(74)
    t = (rs.randint(0, 64, size=(517, 320)) * 2.0 ** -4).astype(np.float32)
    sizes = mc.nondyadic_lists()
    got = mapstats.category_means(_dev(t), sizes).cpu().numpy()
    frame = pd.DataFrame(t.astype(np.float64))
    want = np.stack([frame[c].mean(axis=1).values for c in sizes], axis=1)
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[:, 2]).all() and not np.isnan(got[:, [0, 1, 3]]).any()
    assert np.array_equal(got, mc.category_means(t, sizes), equal_nan=True)
    # a view with ld > G
    assert np.array_equal(mapstats.category_means(_dev(t)[:, :300], [[299, 0]]).cpu().numpy(), mc.category_means(t, [[299, 0]]))


def test_means_on_the_non_dyadic_golden_and_percentiles_of_the_device_means():
    _lib.require_gpu()
    want, lists = mc.golden()["nondyadic_means"], mc.nondyadic_lists()
    means = mapstats.category_means(_dev(mc.nondyadic_table()), lists)
    got = means.cpu().numpy()
    for k, members in enumerate(lists):
        if not members:
            assert np.isnan(got[:, k]).all()
            continue
        rel = float(np.max(np.abs(got[:, k] - want[:, k]) / np.abs(want[:, k])))
        print(f"category of {len(members)} genes: worst relative difference from pandas {rel / U:.2f} x 2^-53, bound {4 * len(members)}")
        assert rel <= 4 * len(members) * U
    perc, first = _percentile(means, return_argmax=True)
    restated = mc.percentile(got)                                  # of the DOWNLOADED means: a last-bit difference may reorder two tiles
    assert np.array_equal(perc, restated, equal_nan=True) and np.array_equal(first, mc.first_argmax(restated))


def test_celltype_maps_equal_the_reference_frame_on_the_dyadic_golden():
    _lib.require_gpu()
    g = mc.golden()
    x, names = mc.dyadic_table()
    xtf, ytf = np.arange(len(x)) % 20, np.arange(len(x)) // 20
    df = mapstats.celltype_maps(_dev(x), names, mc.dyadic_categories(), xtf=xtf, ytf=ytf)
    assert list(df.columns) == ["xcoord_tf", "ycoord_tf", "ac", "ac_perc", "cc", "cc_perc", "mes", "mes_perc", "lin", "lin_perc", "color"]
    assert np.array_equal(df.index.values, g["dyadic_rows"]) and np.array_equal(df["xcoord_tf"].values, xtf[g["dyadic_rows"]])
    assert np.array_equal(df[list(mc.LABELS)].values, g["dyadic_means"])
    assert np.array_equal(df[[label + "_perc" for label in mc.LABELS]].values, g["dyadic_perc"])
    assert df["color"].tolist() == g["dyadic_color"].tolist()
    assert [list(mc.LABELS).index(k) for c in df["color"] for k, v in mc.COLORS.items() if v == c] == g["dyadic_label"].tolist()
    # a table of NaN rows only: the empty frame, nothing launched
    empty = mapstats.celltype_maps(torch.full((3, len(names)), float("nan"), device="cuda"), names, mc.dyadic_categories())
    assert len(empty) == 0 and list(empty.columns)[-1] == "color"


@pytest.mark.parametrize("n,K", mc.CORR_SHAPES)
def test_correlation_against_the_restatement_and_pandas(n, K):
    _lib.require_gpu()
    x = mc.corr_input(n, K)
    out = mapstats.gene_correlation(_dev(x))
    assert out.dtype == torch.float64 and out.shape == (K, K) and out.is_cuda
    got = out.cpu().numpy()
    bound = 4 * n * U
    for what, want in (("restatement", mc.restated_correlation(n, K)), ("DataFrame.corr()", mc.golden()[f"corr_{n}_{K}"])):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        ok = ~np.isnan(want)
        worst = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
        print(f"correlation n={n} K={K} vs {what}: worst difference {worst / U:.2f} x 2^-53, bound {4 * n}")
        assert worst <= bound, what
    assert got.tobytes() == got.T.copy().tobytes()                                   # bit-symmetric
    diag = np.diag(got)
    if (n, K) in mc.CORR_CONSTANT:
        c = mc.CORR_CONSTANT[(n, K)][0]
        assert np.isnan(got[c]).all() and np.isnan(got[:, c]).all() and np.isnan(diag[c]) and int(np.isnan(got).sum()) == 2 * K - 1
        diag = np.delete(diag, c)
    assert np.all(diag == 1.0)
    assert np.nanmax(got) <= 1.0 and np.nanmin(got) >= -1.0


def test_correlation_cols_with_a_wider_table():
    _lib.require_gpu()
    n, K = 1000, 130
    x = mc.corr_input(n, K)
    cols = [128, 3, 77, 3, 129, 64, 0]                                                # a repeat (r = 1 off the diagonal) and the constant column
    got = mapstats.gene_correlation(_dev(x), cols=cols).cpu().numpy()
    want = mc.correlation(x, cols)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[4]).all()
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] - want[ok])) <= 4 * n * U and got[1, 3] == 1.0 and got.tobytes() == got.T.copy().tobytes()
    view = mapstats.gene_correlation(_dev(x)[:, :70]).cpu().numpy()                   # ld = 130 > K = 70, no list
    assert np.max(np.abs(view - mc.restated_correlation(n, K)[:70, :70])) <= 4 * n * U
    first, again = mapstats.gene_correlation(_dev(x)), mapstats.gene_correlation(_dev(x))
    assert first.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()             # two calls, the same bytes


def test_refusals_come_from_the_library_and_launch_nothing():
    _lib.require_gpu()
    L = _lib.lib()
    stream = _lib.stream_ptr("cuda:0")
    x = torch.ones(64, 8, device="cuda")
    out = torch.full((64, 8), -3.0, dtype=torch.float64, device="cuda")
    sq = torch.full((8, 8), -3.0, dtype=torch.float64, device="cuda")
    mo = torch.full((64, 1), -3.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    null = ctypes.c_void_p(0)

    def perc(n=64, C=8, ws_bytes=ws.numel(), f64=0, values=None):
        return L.sq_map_percentile(_lib.ptr(x) if values is None else values, f64, n, 8, null, C, 50.0 / 64, _lib.ptr(out), null, _lib.ptr(ws),
                                   ws_bytes, stream)

    def corr(n=64, K=8, ws_bytes=ws.numel()):
        return L.sq_map_gene_corr(_lib.ptr(x), n, 8, null, K, _lib.ptr(sq), _lib.ptr(ws), ws_bytes, stream)

    def means(n=64, n_cat=1):
        off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
        mem = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
        return L.sq_map_category_means(_lib.ptr(x), n, 8, _lib.ptr(mem), 2, _lib.ptr(off), n_cat, _lib.ptr(mo), stream)

    for call, code, message in ((lambda: perc(n=0), -1, "n = 0 rows"), (lambda: perc(n=262145), -1, "n = 262145 rows"),
                                (lambda: perc(C=0), -1, "C = 0"), (lambda: perc(C=9), -1, "C <= ld"), (lambda: perc(f64=2), -1, "values_f64 = 2"),
                                (lambda: perc(values=null), -1, "null"), (lambda: perc(ws_bytes=1024), -3, "workspace 1024 <"),
                                (lambda: corr(n=1), -1, "n = 1 rows"), (lambda: corr(n=262145), -1, "n = 262145 rows"),
                                (lambda: corr(K=32769), -1, "K = 32769"), (lambda: corr(K=0), -1, "K = 0"),
                                (lambda: corr(ws_bytes=64), -3, "workspace 64 <"),
                                (lambda: means(n=0), -1, "n = 0 rows"), (lambda: means(n=262145), -1, "n = 262145 rows"),
                                (lambda: means(n_cat=0), -1, "n_cat = 0")):
        assert call() == code and message in L.sq_last_error().decode(), (message, L.sq_last_error())
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((sq == -3.0).all()) and bool((mo == -3.0).all()) and not bool(ws.any())      # nothing ran
    assert perc() == 0 and corr() == 0 and means() == 0                                               # the same buffers, good arguments
    torch.cuda.synchronize()
    assert bool((out == 65 * (50.0 / 64)).all()) and bool((mo == 1.0).all()) and bool(torch.isnan(sq).all())       # a table of ones
    # the Python layer: the library's message, or the index check that precedes every upload
    with pytest.raises(_lib.SequoiaHipError, match="n = 0 rows"):
        mapstats.percentile_of_score(torch.zeros(0, 3, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="n = 262145 rows"):
        mapstats.percentile_of_score(torch.zeros(262145, 1, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="n = 1 rows"):
        mapstats.gene_correlation(torch.zeros(1, 3, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="K = 32769"):
        mapstats.gene_correlation(torch.zeros(2, 32769, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="n = 262145 rows"):
        mapstats.category_means(torch.zeros(262145, 2, device="cuda"), [[0]])
    with pytest.raises(ValueError, match="gene index 8 of category 1"):
        mapstats.category_means(x, [[0], [7, 8]])
    with pytest.raises(ValueError, match="column index 8"):
        mapstats.gene_correlation(x, cols=[0, 8])
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        mapstats.gene_correlation(x.cpu())
    with pytest.raises(ValueError):
        mapstats.gene_correlation(x.double())


def test_a_refused_shape_is_the_same_error_from_every_wrapper():
    _lib.require_gpu()
    from sequoia_pub_amd import gtalign
    empty = torch.zeros(0, dtype=torch.float64, device="cuda")
    for call, message in ((lambda: mapstats.percentile_of_score(empty), "n = 0 rows"), (lambda: gtalign.count_unique(empty), "n = 0 rows"),
                          (lambda: mapstats.gene_correlation(torch.zeros(2, 32769, device="cuda")), "K = 32769")):
        with pytest.raises(_lib.SequoiaHipArgError, match=message) as err:
            call()
        assert isinstance(err.value, _lib.SequoiaHipError) and isinstance(err.value, ValueError)


def test_non_default_stream_and_the_largest_row_count():
    _lib.require_gpu()
    x = mc.percentile_input(2 * mapstats.rank_chunk_rows() + 37, 2, np.float32, 56)
    xd = _dev(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        got = _percentile(xd)
    assert np.array_equal(got, mc.percentile(x))
    # SQ_MAP_MAX_ROWS rows of one column: 64 chunks, the counts reach 2^18
    big = (np.random.RandomState(75).randint(0, 1 << 14, mapstats.MAX_ROWS) * 2.0 ** -7).astype(np.float32)
    assert np.array_equal(_percentile(big)[:, 0], mc.percentile(big)[:, 0])


def test_cli_writes_the_three_kinds_of_csv(tmp_path):
    _lib.require_gpu()
    root = str(tmp_path)
    rs = np.random.RandomState(6)
    genes = [f"g{i}" for i in range(70)]
    for name, cols, n in (("s1", genes, 90), ("s2", genes[:40] + genes[45:], 75)):
        df = pd.DataFrame({"xcoord_tf": np.arange(n) % 10, "ycoord_tf": np.arange(n) // 10})
        for c in cols:
            df[c] = (rs.randint(0, 33, n) * 0.125).astype(np.float32)
        df.loc[n - 2, cols[1]] = np.nan
        os.makedirs(os.path.join(root, name))
        df.to_csv(os.path.join(root, name, "stride-1.csv"), index=False)
    os.makedirs(os.path.join(root, "ids"))
    all_genes = genes[::-1][:66] + ["absent"]
    np.save(os.path.join(root, "ids", "all.npy"), np.array(all_genes, dtype=object))
    for k, f in enumerate(cli.CELLTYPE_FILES):
        np.save(os.path.join(root, "ids", f + ".npy"), np.array(genes[4 + 7 * k:4 + 7 * k + 9] + ["nope"], dtype=object))
    total = cli.main(["--pred_folder", root, "--all_genes", os.path.join(root, "ids", "all.npy"), "--celltype_dir", os.path.join(root, "ids")])
    categories = cli.load_categories(os.path.join(root, "ids"))
    lists = cli.cumulative_genes(all_genes, [pd.read_csv(os.path.join(root, s, "stride-1.csv"), nrows=0).columns for s in ("s1", "s2")])
    assert len(lists[0]) == 66 and len(lists[1]) == 61
    frames = []
    for name, corr_genes in zip(("s1", "s2"), lists):
        df = pd.read_csv(os.path.join(root, name, "stride-1.csv")).dropna(axis=0, how="any")
        table = _dev(df[corr_genes].values.astype(np.float32))
        want = pd.DataFrame(mapstats.gene_correlation(table).cpu().numpy(), index=corr_genes, columns=corr_genes)
        got = pd.read_csv(os.path.join(root, "corr_maps", name + "_corr.csv"), index_col=0, float_precision="round_trip")
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        frames.append(want)
        maps = mapstats.celltype_maps(_dev(df[lists[-1]].values.astype(np.float32)), lists[-1], categories, xtf=df["xcoord_tf"].values,
                                      ytf=df["ycoord_tf"].values).reset_index(drop=True)
        got = pd.read_csv(os.path.join(root, "spatial_maps", name + ".csv"), float_precision="round_trip")
        assert len(got) == len(df) and list(got.columns) == list(maps.columns)
        pd.testing.assert_frame_equal(got, maps, check_exact=True)
    want_total = mapstats.mean_correlation(frames)
    got = pd.read_csv(os.path.join(root, "corr_maps", "total_corr.csv"), index_col=0, float_precision="round_trip")
    pd.testing.assert_frame_equal(got, want_total, check_exact=True)
    pd.testing.assert_frame_equal(total, want_total, check_exact=True)
    assert got.shape == (66, 66) and int(got.isna().values.sum()) == 66 * 66 - 61 * 61
