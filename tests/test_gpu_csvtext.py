"""The device CSV text (sequoia_pub_amd.csvtext, csrc/csvtext.hip) against numpy and pandas themselves, byte for byte:
(a) the float32 value list of the host check formatted on the device against ``ndarray.astype(str)``; (b) small frames
against ``DataFrame.to_csv()``; (c) ``sq_fold_mean_f32`` against ``DataFrame.mean(axis=1)``; (d) the capacity guard;
(e) ``cli.visualize --table device`` against ``--table host`` on the synthetic slide of tests/test_gpu_spatial.py, and the
two table paths of the library at a stride below 10 and at stride 10, tiles no window covers included."""
import os
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import csvtext_cases as cc  # noqa: E402
from sequoia_pub_amd import _lib, csvtext  # noqa: E402
from sequoia_pub_amd._abi import CONSTANTS as C  # noqa: E402

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_float32_values_equal_numpy_astype_str():
    """(a) every value of csvtext_cases.f32_bits() as a cell of an 8-column table (the list padded with its first values)."""
    bits, want = cc.f32_bits(), cc.f32_strings()
    cols = 8
    rows = -(-len(bits) // cols)
    assert rows <= csvtext.MAX_TILES
    pad = rows * cols - len(bits)
    table = np.concatenate([bits, bits[:pad]]).view(np.float32).reshape(rows, cols)
    text = want + want[:pad]
    expect = "".join("0," + ",".join(text[r * cols:(r + 1) * cols]) + "\n" for r in range(rows)).encode()
    fm = csvtext.RowFormatter(torch.zeros(rows, dtype=torch.int64, device=DEV), torch.zeros(rows, 0, dtype=torch.int64, device=DEV), _dev(table))
    assert fm.chunk_rows == rows
    fm.format(0, rows)
    total = fm.result()
    got = fm.text[:total].cpu().numpy().tobytes()
    if got != expect:
        g, w = got.decode("ascii", "replace").split("\n"), expect.decode().split("\n")
        bad = [(r, a, b) for r, (a, b) in enumerate(zip(g, w)) if a != b]
        pytest.fail(f"{len(bad)} of {rows} rows differ (lengths {len(got)} and {len(expect)}); the first (row, device, numpy): {bad[:3]}")
    offsets = fm.row_offsets.cpu().numpy()
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(expect, np.uint8) == 10) + 1])
    assert np.array_equal(offsets, starts)


@pytest.mark.parametrize("name", list(cc.frames()))
def test_small_frames_equal_to_csv(name, tmp_path):
    """(b) the file of write_prediction_table against DataFrame.to_csv(), and the returned frame against the frame."""
    df, chunk = cc.frames()[name]
    ints = [c for c in df.columns if df[c].dtype == np.int64]
    floats = [c for c in df.columns if df[c].dtype == np.float32]
    _, _, values = cc.frame_parts(df)
    path = str(tmp_path / "t.csv")
    res, spent = csvtext.write_prediction_table(path, df[ints], _dev(values), floats, chunk_rows=chunk)
    want = df.to_csv().encode()
    assert open(path, "rb").read() == want
    assert spent["bytes"] == len(want) - len(df.iloc[:0].to_csv().encode())
    pd.testing.assert_frame_equal(res, df)


def test_rows_of_a_strided_table_and_a_frame_too_large_to_return(tmp_path):
    """The float columns as a column slice of a wider table (row stride > columns); small=0: no frame comes back."""
    df, _ = cc.frames()["every_third_row_nan"]
    _, _, values = cc.frame_parts(df)
    wide = torch.full((len(df), values.shape[1] + 5), 7.0, device=DEV)
    wide[:, 3:3 + values.shape[1]] = _dev(values)
    path = str(tmp_path / "t.csv")
    res, _ = csvtext.write_prediction_table(path, df[["x"]], wide[:, 3:3 + values.shape[1]], list("abcd"), small=0)
    assert res is None and open(path, "rb").read() == df.to_csv().encode()


@pytest.mark.parametrize("F", [1, 2, 5])
def test_fold_mean_equals_dataframe_mean(F):
    """(c) sq_fold_mean_f32 against DataFrame.mean(axis=1) on float32 columns: equal values, NaN where pandas has NaN, and
    the same sign of zero (np.array_equal does not see that one: the bit patterns are compared as well)."""
    a = cc.fold_tables(F)
    want = cc.pandas_fold_mean(a)
    assert np.isnan(want).any() and (~np.isnan(want)).any()
    got = csvtext.fold_mean(_dev(a)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.signbit(got), np.signbit(want) | (np.isnan(want) & np.signbit(got)))
    # into the columns of a wider table, the folds read from that table: cli.visualize's layout
    n, G = a.shape[1:]
    table = torch.zeros(n, (F + 1) * G, device=DEV)
    table[:, :F * G] = _dev(a).permute(1, 0, 2).reshape(n, F * G)
    csvtext.fold_mean(table[:, :F * G].unflatten(1, (F, G)).permute(1, 0, 2), out=table[:, F * G:])
    assert np.array_equal(table[:, F * G:].cpu().numpy(), want, equal_nan=True)


def test_capacity_one_byte_short_gives_overflow_and_leaves_the_guard_bytes():
    """(d) with a capacity one byte below the text's size the status is SQ_CSV_OVERFLOW, the total is still the size needed,
    every byte from the capacity on keeps its guard value and what lies below the last cell is the text."""
    df, _ = cc.frames()["every_third_row_nan"]
    index, ints, floats = cc.frame_parts(df)
    want = df.to_csv(header=False).encode()
    fm = csvtext.RowFormatter(_dev(index), _dev(ints), _dev(floats))
    assert fm.capacity > len(want) + 64
    fm.text.fill_(0xAB)
    fm.format(0, len(df), capacity=len(want) - 1)
    torch.cuda.synchronize()
    assert int(fm.status.item()) == C["SQ_CSV_OVERFLOW"] and int(fm.total.item()) == len(want)
    with pytest.raises(_lib.SequoiaHipError, match="bytes"):
        fm.result()
    got = fm.text.cpu().numpy()
    assert (got[len(want) - 1:] == 0xAB).all()
    assert got[:len(want) - 1].tobytes() == want[:-1]
    fm.text.fill_(0xAB)
    fm.format(0, len(df), capacity=len(want))                 # exactly enough: the text, and still nothing behind it
    assert fm.result() == len(want)
    got = fm.text.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == 0xAB).all()


def test_refusals():
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="dtype"):
        csvtext.RowFormatter(idx.to(torch.int32), torch.zeros(4, 0, dtype=torch.int64, device=DEV), torch.zeros(4, 1, device=DEV))
    with pytest.raises(ValueError, match="dtype"):
        csvtext.RowFormatter(idx, torch.zeros(4, 0, dtype=torch.int64, device=DEV), torch.zeros(4, 1, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="at most"):
        n = csvtext.MAX_TILES + 1
        csvtext.RowFormatter(torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, 0, dtype=torch.int64, device=DEV), torch.zeros(n, 1, device=DEV))
    with pytest.raises(ValueError, match="int64"):
        csvtext.write_prediction_table("unused.csv", pd.DataFrame({"x": [1.5]}), torch.zeros(1, 1, device=DEV), ["g"])
    assert "int64" in csvtext.frame_refusal(pd.DataFrame({"x": [1]}, index=["a"]), ["g"])
    with pytest.raises(ValueError, match="folds"):
        csvtext.fold_mean(torch.zeros(csvtext.MAX_FOLDS + 1, 2, 2, device=DEV))


# ---- (e) the two table paths ------------------------------------------------------------------------------------------------

def _host_table(df, tile_features, models, genes, names, stride, path):
    """cli/visualize.py's host path for these folds: sliding_window_method, Index.map per gene and fold, mean, to_csv."""
    from sequoia_pub_amd.spatial import sliding_window_method
    res_df = df.copy(deep=True)
    folds = list(range(len(models)))
    for fold, model in zip(folds, models):
        preds = sliding_window_method(df, tile_features, model, genes, stride)
        for g in genes:
            res_df[names[g] + '_' + str(fold)] = res_df.index.map(preds[g])
    for g in genes:
        res_df[names[g]] = res_df[[names[g] + '_' + str(i) for i in folds]].mean(axis=1)
    res_df.to_csv(path)
    return res_df


def _fold_models(model_type, G, input_dim):
    """Two folds of the aggregator on the device, seeded."""
    from sequoia_pub_amd.he2rna import HE2RNA
    from sequoia_pub_amd.vis import ViS
    models = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        if model_type == "vis":
            m = ViS(G, input_dim, 2, 4, 64, 64, 64, device="cpu")
        else:
            m = HE2RNA(input_dim=input_dim, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], output_dim=G, device="cpu")
            m.device = DEV
        models.append(m.to(DEV).eval())
    return models


@pytest.mark.parametrize("stride", [3, 10])
@pytest.mark.parametrize("model_type", ["vis", "he2rna"])
def test_library_table_paths_write_the_same_bytes(model_type, stride, tmp_path):
    """A 14 x 9 tile grid plus a detached clump that no kept window covers, two folds of ViS and of HE2RNA (which takes its
    own route, per-tile scores and a vote on window predictions per tile chunk): the dictionaries of sliding_window_method
    assembled as cli.visualize does on the host, against sliding_window_table + fold_mean + write_prediction_table.
    stride 3: means over windows; stride 10: last writer, and the columns 10..13 of the grid lie in no kept window (36
    tiles), so whole rows are empty cells."""
    from sequoia_pub_amd.spatial import sliding_window_table
    _lib.require_gpu()
    xy = [(x, y) for x in range(14) for y in range(9)] + [(30, 0), (30, 1), (31, 0)]
    df = pd.DataFrame({"xcoord": [256 * x for x, _ in xy], "ycoord": [256 * y for _, y in xy], "xcoord_tf": [x for x, _ in xy], "ycoord_tf": [y for _, y in xy]})
    assert all(df[c].dtype == np.int64 for c in df.columns)
    G, genes = 12, [7, 2, 11]
    names = [f"G{i}" for i in range(G)]
    feats = torch.randn(len(df), 256, generator=torch.Generator().manual_seed(5)).to(DEV)
    models = _fold_models(model_type, G, 256)
    host = _host_table(df, feats, models, genes, names, stride, str(tmp_path / "host.csv"))
    F, S = len(models), len(genes)
    table = torch.empty(len(df), (F + 1) * S, device=DEV)
    for k, m in enumerate(models):
        table[:, k * S:(k + 1) * S] = sliding_window_table(df, feats, m, genes, stride)
    csvtext.fold_mean(table[:, :F * S].unflatten(1, (F, S)).permute(1, 0, 2), out=table[:, F * S:])
    cols = [names[g] + '_' + str(f) for f in range(F) for g in genes] + [names[g] for g in genes]
    res, _ = csvtext.write_prediction_table(str(tmp_path / "device.csv"), df, table, cols)
    want = open(tmp_path / "host.csv", "rb").read()
    assert open(tmp_path / "device.csv", "rb").read() == want
    assert host[names[genes[0]]].isna().sum() == (3 if stride == 3 else 3 + 36) and want.count(b",,") > 0
    pd.testing.assert_frame_equal(res, host)


@pytest.fixture(scope="module")
def synthetic_slide(tmp_path_factory):
    """The slide, mask, extractor weights and fold checkpoints of tests/test_gpu_spatial.py's CLI test."""
    from oracle import resnet_oracle
    from sequoia_pub_amd.he2rna import HE2RNA
    from sequoia_pub_amd.resnet import resnet50
    from sequoia_pub_amd.vis import ViS
    _lib.require_gpu()
    root = str(tmp_path_factory.mktemp("csvtext_cli"))
    rs = np.random.RandomState(4)
    nx, ny, G = 9, 8, 24
    arr = rs.randint(0, 256, ((ny + 1) * 256, (nx + 1) * 256, 3), dtype=np.uint8)
    os.makedirs(os.path.join(root, "TCGA", "P"))
    np.save(os.path.join(root, "TCGA", "P", "TCGA-X.npy"), arr)
    mask = np.ones(((nx + 1) * 8, (ny + 1) * 8), dtype=bool)
    mask[:, 56:] = False
    np.save(os.path.join(root, "mask.npy"), mask)
    genes = [f"G{i}" for i in range(G)]
    rw = os.path.join(root, "resnet.pth")
    torch.save({**resnet50().state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3)}, rw)
    for mt in ("vis", "he2rna"):
        ck = os.path.join(root, f"{mt}_resnet", "st")
        os.makedirs(ck)
        pickle.dump({"genes": genes}, open(os.path.join(ck, "test_results.pkl"), "wb"))
        torch.manual_seed(7)
        for fold in (0, 1):
            if mt == "vis":
                m = ViS(G, 2048, 6, 16, 64, 64, 64, device="cpu")
                torch.save(m.state_dict(), os.path.join(ck, "model_best.pt" if fold == 0 else f"model_best_{fold}.pt"))
            else:
                m = HE2RNA(input_dim=2048, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], output_dim=G)
                torch.save(m, os.path.join(ck, f"model_{fold}.pt"))
    common = ["--study", "st", "--project", "P", "--gene_names", "G3,G17,nope,G3", "--wsi_file_name", "TCGA-X.npy", "--save_folder", "t",
              "--feat_type", "resnet", "--slide_path", os.path.join(root, "TCGA", "P"), "--mask_path", os.path.join(root, "mask.npy"),
              "--extractor_weights", rw, "--compute_dtype", "fp32"]
    return root, common, nx * (ny - 1)


@pytest.mark.parametrize("model_type,folds", [("vis", "0,1"), ("he2rna", "0,1")])
def test_visualize_cli_table_device_writes_the_host_file(synthetic_slide, model_type, folds):
    """(e) cli.visualize --table device and --table host (the default) write byte-identical files, and the small frame that
    comes back is the host's; a gene named twice is one column in both."""
    from sequoia_pub_amd.cli import visualize
    root, common, n_tiles = synthetic_slide
    args = common + ["--model_type", model_type, "--folds", folds, "--checkpoint", os.path.join(root, f"{model_type}_resnet", "st")]
    res_h, path_h = visualize.main(args + ["--out_root", os.path.join(root, f"host_{model_type}")])
    res_d, path_d = visualize.main(args + ["--out_root", os.path.join(root, f"device_{model_type}"), "--table", "device"])
    want = open(path_h, "rb").read()
    assert path_h != path_d and open(path_d, "rb").read() == want
    assert len(res_h) == n_tiles and want.count(b"\n") == n_tiles + 1
    assert list(res_h.columns) == ["xcoord", "ycoord", "xcoord_tf", "ycoord_tf", "G3_0", "G17_0", "G3_1", "G17_1", "G3", "G17"]
    pd.testing.assert_frame_equal(res_d, res_h)
