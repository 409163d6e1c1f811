"""What the device map statistics can be held to without a GPU: the numpy restatement of tests/mapstats_cases.py equals the
reference's literal calls on every golden case (tests/golden/mapstats.npz), the command line's grouping, skipping and
cumulative-intersection logic on frames with the three device calls stubbed by the restatement, the argument checks that
need no device, and the built library's new symbols."""
import os
import zlib
from collections import OrderedDict

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.stats import percentileofscore

import mapstats_cases as mc
from sequoia_pub_amd import _lib, mapstats
from sequoia_pub_amd.cli import gbm_celltype_analysis as cli

U = 2.0 ** -53


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _stub_percentile(values, cols=None, return_argmax=False):
    p = mc.percentile(values.numpy(), cols)
    return (torch.from_numpy(p), torch.from_numpy(mc.first_argmax(p))) if return_argmax else torch.from_numpy(p)


def _stub_means(pred, categories):
    lists = list(categories.values()) if hasattr(categories, "values") else list(categories)
    return torch.from_numpy(mc.category_means(pred.numpy(), lists))


def _stub_corr(pred, cols=None):
    return torch.from_numpy(mc.correlation(pred.numpy(), cols))


@pytest.fixture
def stubbed(monkeypatch):
    monkeypatch.setattr(mapstats, "percentile_of_score", _stub_percentile)
    monkeypatch.setattr(mapstats, "category_means", _stub_means)
    monkeypatch.setattr(mapstats, "gene_correlation", _stub_corr)


def test_golden_inputs_are_the_ones_the_file_was_made_from():
    g = mc.golden()
    for name in mc.GOLDEN_PERC:
        assert _crc(mc.golden_percentile_input(name)) == int(g[name + "_crc"][0]), name
    assert _crc(mc.dyadic_table()[0]) == int(g["dyadic_crc"][0]) and _crc(mc.nondyadic_table()) == int(g["nondyadic_crc"][0])
    for n, K in mc.CORR_SHAPES:
        assert _crc(mc.corr_input(n, K)) == int(g[f"corr_{n}_{K}_crc"][0]), (n, K)


@pytest.mark.parametrize("name", list(mc.GOLDEN_PERC))
def test_restated_percentile_equals_scipy_row_by_row(name):
    x, want = mc.golden_percentile_input(name), mc.golden()[name + "_out"]
    got = mc.percentile(x)
    assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(want[:, -1]).all() and not np.isnan(want[:, :-1]).any()           # the NaN column, and only it
    assert len(np.unique(want[:, 1])) == 1                                           # the constant column: every tile mid-rank
    assert np.isinf(x).any() and (np.signbit(x) & (x == 0)).any()
    a = x[:, 0]                                                                       # and three literal calls, here
    for i in (0, len(a) // 2, len(a) - 1):
        assert got[i, 0] == percentileofscore(a, a[i])


def test_restated_means_percentiles_and_labels_equal_the_reference_frame_on_the_dyadic_table():
    g = mc.golden()
    x, names = mc.dyadic_table()
    rows = np.flatnonzero(~np.isnan(x).any(axis=1))
    assert np.array_equal(rows, g["dyadic_rows"]) and len(rows) == mc.DYADIC_SHAPE[0] - len(mc.DYADIC_NAN_ROWS)
    lists = list(mapstats.category_indices(names, mc.dyadic_categories()).values())
    assert [len(c) for c in lists] == [3, 8, 5, 16]
    means = mc.category_means(x[rows], lists)
    perc = mc.percentile(means)
    assert np.array_equal(means, g["dyadic_means"]) and np.array_equal(perc, g["dyadic_perc"])
    assert np.array_equal(mc.first_argmax(perc), g["dyadic_label"])
    assert len(set(g["dyadic_label"].tolist())) == 4
    assert int((np.sort(perc, axis=1)[:, -1] == np.sort(perc, axis=1)[:, -2]).sum()) >= 1, "no tile with tied leading percentiles"


def test_restated_means_are_within_the_summation_bound_of_pandas_on_the_non_dyadic_table():
    want = mc.golden()["nondyadic_means"]
    lists = mc.nondyadic_lists()
    got = mc.category_means(mc.nondyadic_table(), lists)
    assert [len(c) for c in lists] == [1, 7, 0, 300]
    for k, members in enumerate(lists):
        if not members:
            assert np.isnan(got[:, k]).all() and np.isnan(want[:, k]).all()
        else:
            assert np.all(np.abs(got[:, k] - want[:, k]) <= 4 * len(members) * U * np.abs(want[:, k])), k


@pytest.mark.parametrize("n,K", mc.CORR_SHAPES)
def test_restated_correlation_is_within_the_dot_product_bound_of_pandas(n, K):
    want, got = mc.golden()[f"corr_{n}_{K}"], mc.restated_correlation(n, K)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 4 * n * U)
    if (n, K) in mc.CORR_CONSTANT:
        c = mc.CORR_CONSTANT[(n, K)][0]
        assert np.isnan(want[c]).all() and np.isnan(want[:, c]).all() and int(np.isnan(want).sum()) == 2 * K - 1
    else:
        assert ok.all()


def test_celltype_maps_on_the_dyadic_golden_with_stubbed_device_calls(stubbed):
    g = mc.golden()
    x, names = mc.dyadic_table()
    xtf = np.arange(len(x)) % 20
    ytf = np.arange(len(x)) // 20
    df = mapstats.celltype_maps(torch.from_numpy(x.copy()), names, mc.dyadic_categories(), xtf=xtf, ytf=ytf)
    assert list(df.columns) == ["xcoord_tf", "ycoord_tf", "ac", "ac_perc", "cc", "cc_perc", "mes", "mes_perc", "lin", "lin_perc", "color"]
    assert np.array_equal(df.index.values, g["dyadic_rows"])
    assert np.array_equal(df["xcoord_tf"].values, xtf[g["dyadic_rows"]]) and np.array_equal(df["ycoord_tf"].values, ytf[g["dyadic_rows"]])
    assert np.array_equal(df[list(mc.LABELS)].values, g["dyadic_means"])
    assert np.array_equal(df[[label + "_perc" for label in mc.LABELS]].values, g["dyadic_perc"])
    assert df["color"].tolist() == g["dyadic_color"].tolist()
    assert mapstats.COLORS == OrderedDict((k, mc.COLORS[k]) for k in mc.LABELS)


def test_cli_grouping_and_cumulative_gene_lists():
    lists = {f: [f + "_a", f + "_b"] for f in cli.CELLTYPE_FILES}
    lists["G2M"] = ["G1S_a", "G2M_b"]                                    # a gene in two lists stays twice
    cats = cli.group_categories(lists)
    assert list(cats) == ["ac", "cc", "mes", "lin"]
    assert cats["ac"] == ["AC_a", "AC_b"] and cats["cc"] == ["G1S_a", "G1S_b", "G1S_a", "G2M_b"]
    assert cats["mes"] == ["MES1_a", "MES1_b", "MES2_a", "MES2_b"] and len(cats["lin"]) == 6 and cats["lin"][4:] == ["OPC_a", "OPC_b"]
    got = cli.cumulative_genes(["g3", "g1", "g2", "g0"], [["x", "g0", "g1", "g3"], ["g3", "g2", "g0", "y"], ["g0", "g3", "g1"]])
    assert got == [["g3", "g1", "g0"], ["g3", "g0"], ["g3", "g0"]]          # the order of all.npy, shrinking


def _write_slides(root, rs):
    """Two slides: the second lacks two genes of all.npy and holds a row with a NaN in a column that is no listed gene."""
    genes = [f"g{i}" for i in range(12)]
    frames = {}
    for name, cols, n in (("slideA", genes + ["extra"], 37), ("slideB", [g for g in genes if g not in ("g2", "g9")] + ["extra"], 29)):
        df = pd.DataFrame({"xcoord_tf": np.arange(n) % 7, "ycoord_tf": np.arange(n) // 7})
        for c in cols:
            df[c] = (rs.randint(0, 9, n) * 0.25 + rs.randint(0, 4, n) * 2.0 ** -5).astype(np.float32)
        df.loc[3, "extra"] = np.nan
        os.makedirs(os.path.join(root, name))
        df.to_csv(os.path.join(root, name, "stride-1.csv"), index=False)
        frames[name] = df
    os.makedirs(os.path.join(root, "ids"))
    np.save(os.path.join(root, "ids", "all.npy"), np.array(["g5", "g2", "g0", "absent", "g9", "g1", "g11", "g7"], dtype=object))
    lists = {"AC": ["g5", "g0", "nope"], "G1S": ["g1"], "G2M": ["g1", "g2"], "MES1": ["g7", "g9"], "MES2": ["g11"], "NPC1": [], "NPC2": ["g5"],
             "OPC": ["g0", "g7", "g3"]}                                      # g3 is in the slides but not in all.npy: skipped
    for f, v in lists.items():
        np.save(os.path.join(root, "ids", f + ".npy"), np.array(v, dtype=object))
    return frames


def _literal_flow(root, names):
    """gbm_celltype_analysis.py:60-75, :91-111 and :137-140, with the list order of all.npy in place of set order."""
    all_genes = np.load(os.path.join(root, "ids", "all.npy"), allow_pickle=True).tolist()
    load = lambda f: np.load(os.path.join(root, "ids", f + ".npy"), allow_pickle=True)      # noqa: E731
    ac, g1s, g2m, mes1, mes2, npc1, npc2, opc = (load(f) for f in cli.CELLTYPE_FILES)
    corrs, maps = [], {}
    for name in names:
        df = pd.read_csv(os.path.join(root, name, "stride-1.csv"))
        all_genes = [g for g in all_genes if g in set(df.columns)]
        df = df.dropna(axis=0, how="any")
        df = df[["xcoord_tf", "ycoord_tf"] + all_genes]
        corrs.append(df[all_genes].corr())
    for name in names:
        df = pd.read_csv(os.path.join(root, name, "stride-1.csv"))
        all_genes = [g for g in all_genes if g in set(df.columns)]
        df = df.dropna(axis=0, how="any")
        df = df[["xcoord_tf", "ycoord_tf"] + all_genes]
        categories = [ac.tolist(), g1s.tolist() + g2m.tolist(), mes1.tolist() + mes2.tolist(), npc1.tolist() + npc2.tolist() + opc.tolist()]
        labels = ["ac", "cc", "mes", "lin"]
        for j, label in enumerate(labels):
            df[label] = df[[i for i in categories[j] if i in df.columns]].mean(axis=1)
            ref = df[label].values
            df[label + "_perc"] = df.apply(lambda row: percentileofscore(ref, row[label]), axis=1)
        df["color"] = df[[i + "_perc" for i in labels]].idxmax(axis=1)
        df["color"] = df["color"].str.replace("_perc", "")
        df["color"] = df["color"].map(mc.COLORS)
        maps[name] = df
    total = corrs[0].copy()
    for c in corrs[1:]:
        total += c
    return corrs, maps, total / len(corrs)


def test_cli_files_equal_the_literal_flow_with_stubbed_device_calls(tmp_path, stubbed):
    root = str(tmp_path)
    _write_slides(root, np.random.RandomState(5))
    total = cli.main(["--pred_folder", root, "--all_genes", os.path.join(root, "ids", "all.npy"), "--celltype_dir", os.path.join(root, "ids"),
                      "--device", "cpu"])
    names = ["slideA", "slideB"]
    assert cli.slide_names(root) == names                                  # ids/, corr_maps/ and spatial_maps/ are no slides
    corrs, maps, want_total = _literal_flow(root, names)
    assert list(corrs[0].columns) == ["g5", "g2", "g0", "g9", "g1", "g11", "g7"] and list(corrs[1].columns) == ["g5", "g0", "g1", "g11", "g7"]
    for name, want in zip(names, corrs):
        got = pd.read_csv(os.path.join(root, "corr_maps", name + "_corr.csv"), index_col=0, float_precision="round_trip")
        assert list(got.columns) == list(want.columns) and list(got.index) == list(want.index)
        assert np.all(np.abs(got.values - want.values) <= 4 * 28 * U)
    got_total = pd.read_csv(os.path.join(root, "corr_maps", "total_corr.csv"), index_col=0, float_precision="round_trip")
    assert sorted(got_total.columns) == sorted(want_total.columns) and got_total.shape == (7, 7)
    want_total = want_total.loc[got_total.index, got_total.columns]
    assert np.array_equal(np.isnan(got_total.values), np.isnan(want_total.values)) and int(np.isnan(got_total.values).sum()) == 49 - 25
    ok = ~np.isnan(want_total.values)
    assert np.all(np.abs(got_total.values[ok] - want_total.values[ok]) <= 4 * 28 * U)
    pd.testing.assert_frame_equal(total, got_total, check_exact=False, rtol=0, atol=1e-15)
    columns = ["xcoord_tf", "ycoord_tf", "ac", "ac_perc", "cc", "cc_perc", "mes", "mes_perc", "lin", "lin_perc", "color"]
    for name in names:
        got = pd.read_csv(os.path.join(root, "spatial_maps", name + ".csv"), float_precision="round_trip")      # the default parser is a few ulp off
        want = maps[name][columns].reset_index(drop=True)
        assert list(got.columns) == columns and len(got) == len(want) == (36 if name == "slideA" else 28)
        for c in columns[:-1]:
            assert np.array_equal(got[c].values.astype(np.float64), want[c].values.astype(np.float64)), (name, c)
        assert got["color"].tolist() == want["color"].tolist()


def test_mean_correlation_aligns_by_label():
    a = pd.DataFrame([[1.0, 0.5], [0.5, 1.0]], index=["x", "y"], columns=["x", "y"])
    b = pd.DataFrame([[1.0, -0.5], [-0.5, 1.0]], index=["y", "x"], columns=["y", "x"])
    got = mapstats.mean_correlation([a, b])
    assert got.loc["x", "y"] == 0.0 and got.loc["x", "x"] == 1.0 and a.loc["x", "y"] == 0.5          # the inputs are left alone
    with pytest.raises(ValueError):
        mapstats.mean_correlation([])


def test_gene_indices_are_validated_before_anything_is_uploaded():
    with pytest.raises(ValueError, match="gene index 40 of category 1"):
        mapstats._category_lists([[0, 1], [3, 40]], 40)
    with pytest.raises(ValueError, match="gene index -1"):
        mapstats._category_lists({"a": [-1]}, 40)
    members, offsets = mapstats._category_lists(OrderedDict([("a", [3, 3, 1]), ("b", []), ("c", [39])]), 40)
    assert members.tolist() == [3, 3, 1, 39] and offsets.tolist() == [0, 3, 3, 4] and members.dtype == offsets.dtype == np.int32
    with pytest.raises(ValueError, match="column index 7"):
        mapstats._columns([0, 7], 7, "cpu", "gene_correlation")
    assert mapstats.category_indices(["a", "b", "a"], {"k": ["b", "zz", "a", "b"]}) == {"k": [1, 0, 1]}


def test_cpu_tensor_raises_not_falls_back():
    x = torch.zeros(8, 4)
    for call in (lambda: mapstats.percentile_of_score(x), lambda: mapstats.category_means(x, [[0]]), lambda: mapstats.gene_correlation(x)):
        with pytest.raises(_lib.SequoiaHipError):
            call()


def test_a_refused_argument_is_a_library_error_and_a_value_error():
    assert issubclass(_lib.SequoiaHipArgError, _lib.SequoiaHipError) and issubclass(_lib.SequoiaHipArgError, ValueError)
    L = _lib.lib()
    assert L.sq_map_category_means(None, 0, 1, None, 0, None, 1, None, None) == -1          # refused before any pointer is looked at
    with pytest.raises(_lib.SequoiaHipArgError, match="libsequoia_hip error -1: map_category_means: n = 0 rows"):
        _lib.check(-1)
    with pytest.raises(_lib.SequoiaHipError) as other:
        _lib.check(-3)
    assert not isinstance(other.value, ValueError)


def test_library_exports_the_map_statistics():
    L = _lib.lib()
    for name in ("sq_map_rank_chunk_rows", "sq_map_percentile_workspace_bytes", "sq_map_percentile", "sq_map_category_means",
                 "sq_map_gene_corr_workspace_bytes", "sq_map_gene_corr"):
        assert hasattr(L, name), name
    c = mapstats.rank_chunk_rows()
    assert c >= 256 and c & (c - 1) == 0
    # the size functions are host arithmetic: 0 for every refused shape
    assert L.sq_map_percentile_workspace_bytes(0, 1, 0) == 0 and L.sq_map_percentile_workspace_bytes(mapstats.MAX_ROWS + 1, 1, 0) == 0
    assert L.sq_map_percentile_workspace_bytes(5, 0, 1) == 0 and L.sq_map_percentile_workspace_bytes(5, 1, 2) == 0
    assert L.sq_map_percentile_workspace_bytes(c + 1, 3, 1) >= 3 * 2 * c * 8 and L.sq_map_percentile_workspace_bytes(mapstats.MAX_ROWS, 1, 0) > 0
    assert L.sq_map_gene_corr_workspace_bytes(1, 4) == 0 and L.sq_map_gene_corr_workspace_bytes(mapstats.MAX_ROWS + 1, 4) == 0
    assert L.sq_map_gene_corr_workspace_bytes(100, 0) == 0 and L.sq_map_gene_corr_workspace_bytes(100, mapstats.MAX_CORR_COLS + 1) == 0
    assert L.sq_map_gene_corr_workspace_bytes(2, 1) > 0 and L.sq_map_gene_corr_workspace_bytes(mapstats.MAX_ROWS, mapstats.MAX_CORR_COLS) > 0
