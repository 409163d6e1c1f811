"""sequoia_pub_amd.mapstats.row_distances / linkage_average / cluster_order (csrc/linkage.hip) on the device against the numpy
restatement of tests/linkage_cases.py and scipy's own results in tests/golden/linkage.npz.  Every comparison is equality
of bytes: the distances, Z and the leaves are what scipy gives, ties and zero distances included."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import linkage_cases as lc  # noqa: E402
from sequoia_pub_amd import _lib, mapstats  # noqa: E402
from sequoia_pub_amd.cli import gbm_celltype_analysis as cli  # noqa: E402

SENTINEL = -3.0


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _device_results(A):
    """A: a device tensor -> (dist, Z, leaves) downloaded."""
    D = mapstats.row_distances(A)
    Z, lv = mapstats.linkage_average(A)
    assert D.dtype == torch.float64 and Z.dtype == torch.float64 and lv.dtype == torch.int32 and D.is_cuda and Z.is_cuda and lv.is_cuda
    return D.cpu().numpy(), Z.cpu().numpy(), lv.cpu().numpy()


def _assert_case(name, got):
    D, Z, lv = got
    wD, wZ, wlv, _ = lc.restated(name)
    g = lc.golden()
    K = wD.shape[0]
    assert D.shape == (K, K) and Z.shape == (K - 1, 4) and lv.shape == (K,)
    print(f"{name}: {int((D != wD).sum())} of {D.size} distances, {int((Z != wZ).sum())} of {Z.size} Z entries, {int((lv != wlv).sum())} of {K} leaves differ")
    assert D.tobytes() == wD.tobytes()
    assert Z.tobytes() == wZ.tobytes() and Z.tobytes() == g[name + "_Z"].tobytes()
    assert lv.tobytes() == wlv.tobytes() and lv.tobytes() == g[name + "_leaves"].tobytes()
    if K <= lc.GOLDEN_DIST_MAX_K:
        assert lc.condensed(D).tobytes() == g[name + "_pdist"].tobytes()
    else:
        assert lc.digest(lc.condensed(D)) == str(g[name + "_pdist_sha256"])
    assert D.tobytes() == D.T.copy().tobytes() and not D.diagonal().any()


@pytest.mark.parametrize("name", [f"corr_{K}" for K in lc.SIZES] + [f"rect_{K}x8" for K in lc.SEARCH_STEP] + [f"rect_{lc.BOUND}x4"])
def test_sizes_are_bit_equal_to_the_restatement_and_scipy(name):
    _lib.require_gpu()
    _assert_case(name, _device_results(_dev(lc.case(name))))


@pytest.mark.parametrize("name", lc.TIES)
def test_ties_and_zero_distances_follow_scipy(name):
    _lib.require_gpu()
    _assert_case(name, _device_results(_dev(lc.case(name))))


def test_rectangular_observations_and_a_wider_leading_dimension():
    _lib.require_gpu()
    A = lc.case("rect_33x8")
    _assert_case("rect_33x8", _device_results(_dev(A)))
    wide = torch.full((33, 11), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :8] = _dev(A)
    view = wide[:, :8]
    assert view.stride(0) == 11 and not view.is_contiguous()
    _assert_case("rect_33x8", _device_results(view))


def test_a_batch_equals_the_single_calls_byte_for_byte():
    _lib.require_gpu()
    names = ("rect_33x8", "repeated_33x8", "rect_33x8")
    batch = _dev(np.stack([lc.case(n) for n in names]))
    batch[2] = batch[2].flip(0)                                  # a third problem of its own
    D, (Z, lv) = mapstats.row_distances(batch), mapstats.linkage_average(batch)
    assert D.shape == (3, 33, 33) and Z.shape == (3, 32, 4) and lv.shape == (3, 33)
    for b in range(3):
        sD, sZ, slv = _device_results(batch[b].clone())
        assert D[b].cpu().numpy().tobytes() == sD.tobytes() and Z[b].cpu().numpy().tobytes() == sZ.tobytes()
        assert lv[b].cpu().numpy().tobytes() == slv.tobytes()
    for b in (0, 1):
        _assert_case(names[b], (D[b].cpu().numpy(), Z[b].cpu().numpy(), lv[b].cpu().numpy()))
    third = lc.linkage(np.array(lc.case("rect_33x8"))[::-1])
    assert Z[2].cpu().numpy().tobytes() == third[1].tobytes() and lv[2].cpu().numpy().tobytes() == third[2].tobytes()


def test_non_default_stream_and_two_calls_give_the_same_bytes():
    _lib.require_gpu()
    A = _dev(lc.case("corr_130"))
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        first = _device_results(A)
    _assert_case("corr_130", first)
    again = _device_results(A)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))


def _raw(A, K, M, B=1, ld=None, a_ptr=None, ws_dist=None, ws_link=None):
    """The two entries called directly on sentinel-filled outputs -> (codes, messages, dist, status [2, B], Z, leaves)."""
    L = _lib.lib()
    stream = _lib.stream_ptr("cuda:0")
    Kc, Bc = min(max(K, 2), 64), max(B, 1)
    dist = torch.full((Bc, Kc, Kc), SENTINEL, dtype=torch.float64, device="cuda")
    Z = torch.full((Bc, Kc - 1, 4), SENTINEL, dtype=torch.float64, device="cuda")
    leaves = torch.full((Bc, Kc), -7, dtype=torch.int32, device="cuda")
    status = torch.full((2, Bc), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    codes, messages = [], []
    codes.append(L.sq_map_row_distances(_lib.ptr(A) if a_ptr is None else a_ptr, B, K, M, M if ld is None else ld, _lib.ptr(dist), _lib.ptr(status[0]),
                                        _lib.ptr(ws), ws.numel() if ws_dist is None else ws_dist, stream))
    messages.append(L.sq_last_error().decode())
    codes.append(L.sq_map_linkage_average(_lib.ptr(dist), B, K, _lib.ptr(status[0]), _lib.ptr(Z), _lib.ptr(leaves), _lib.ptr(status[1]),
                                          _lib.ptr(ws), ws.numel() if ws_link is None else ws_link, stream))
    messages.append(L.sq_last_error().decode())
    torch.cuda.synchronize()
    return codes, messages, dist, status, Z, leaves


def test_a_nan_row_and_column_set_the_status_and_raise():
    _lib.require_gpu()
    c = np.array(lc.case("corr_17"))
    c[5, :] = np.nan
    c[:, 5] = np.nan
    codes, _, dist, status, Z, leaves = _raw(_dev(c), 17, 17)
    assert codes == [0, 0]
    assert status.cpu().numpy().tolist() == [[1 + lc.first_nonfinite_row(lc.row_distances(c))], [mapstats._C["SQ_LINK_NONFINITE"]]]
    assert bool((Z == SENTINEL).all()) and bool((leaves == -7).all())                      # the linkage left its outputs alone
    with pytest.raises(ValueError, match="row 0 has a distance that is not finite"):
        mapstats.linkage_average(_dev(c))
    with pytest.raises(ValueError, match="row 0 has a distance that is not finite"):
        mapstats.row_distances(_dev(c))
    # one infinite entry in row 3: the first row with a bad pair is row 0
    r = np.array(lc.case("rect_33x8"))
    r[3, 2] = np.inf
    with pytest.raises(ValueError, match="row 0 has a distance"):
        mapstats.linkage_average(_dev(r))
    batch = np.stack([lc.case("rect_33x8"), r])
    with pytest.raises(ValueError, match="of problem 1"):
        mapstats.linkage_average(_dev(batch))
    _assert_case("corr_17", _device_results(_dev(lc.case("corr_17"))))                     # the next call on good input works


def _raw_linkage(D):
    """sq_map_linkage_average alone on a square distance matrix, dist_status = NULL -> (code, status, Z, leaves)."""
    L = _lib.lib()
    K = D.shape[0]
    dist = _dev(D)
    Z = torch.full((K - 1, 4), SENTINEL, dtype=torch.float64, device="cuda")
    leaves = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    need = int(L.sq_map_linkage_average_workspace_bytes(1, K))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    code = L.sq_map_linkage_average(_lib.ptr(dist), 1, K, ctypes.c_void_p(0), _lib.ptr(Z), _lib.ptr(leaves), _lib.ptr(status), _lib.ptr(ws), need,
                                    _lib.stream_ptr("cuda:0"))
    torch.cuda.synchronize()
    return code, int(status.item()), Z.cpu().numpy(), leaves.cpu().numpy()


def test_the_linkage_without_status_words_checks_the_distances_it_searches():
    """dist_status = NULL: a good matrix gives scipy's Z; a NaN, infinite or negative distance to a live cluster ends the
    problem with SQ_LINK_BAD_DISTANCE before any index comes from it, and Z and the leaves keep their fill."""
    _lib.require_gpu()
    bad_status = mapstats._C["SQ_LINK_BAD_DISTANCE"]
    for name in ("corr_17", "repeated_33x8", "corr_130"):
        wD, wZ, wlv, _ = lc.restated(name)
        code, status, Z, leaves = _raw_linkage(wD)
        assert (code, status) == (0, 0) and Z.tobytes() == wZ.tobytes() and leaves.tobytes() == wlv.tobytes()
    good = np.array(lc.restated("corr_17")[0])
    nan_row = good.copy()                                        # a constant gene: its row and column are NaN, the diagonal 0
    nan_row[5, :] = nan_row[:, 5] = np.nan
    nan_row[5, 5] = 0.0
    everything = np.full((17, 17), np.nan)                       # no candidate ever compares below another
    last = good.copy()                                           # met late: only the pair of the two largest indices
    last[15, 16] = last[16, 15] = np.nan
    inf_pair, negative = good.copy(), good.copy()
    inf_pair[2, 9] = inf_pair[9, 2] = np.inf
    negative[0, 1] = negative[1, 0] = -1.0
    for D in (nan_row, everything, last, inf_pair, negative, np.full((2, 2), np.nan)):
        code, status, Z, leaves = _raw_linkage(D)
        assert (code, status) == (0, bad_status)
        assert bool((Z == SENTINEL).all()) and bool((leaves == -7).all())
    code, status, Z, _ = _raw_linkage(good)                      # the next call on good input works
    assert (code, status) == (0, 0) and Z.tobytes() == lc.restated("corr_17")[1].tobytes()


def test_refusals_come_from_the_library_and_launch_nothing():
    _lib.require_gpu()
    L = _lib.lib()
    bound = mapstats.MAX_LINK_ROWS
    assert bound == 4096 and L.sq_map_row_distances_workspace_bytes(1, bound, 3) > 0 and L.sq_map_linkage_average_workspace_bytes(1, bound) > 0
    A = _dev(lc.case("rect_33x8"))
    null = ctypes.c_void_p(0)
    for kw, which, code, message in ((dict(K=1), (0, 1), -1, "K = 1 rows, must be in 2..4096"), (dict(K=bound + 1), (0, 1), -1, f"K = {bound + 1} rows, must be in 2..4096"),
                                     (dict(M=0), (0,), -1, "M = 0 features"), (dict(B=0), (0, 1), -1, "B = 0 problems"),
                                     (dict(ld=7), (0,), -1, "ld = 7 for M = 8"), (dict(a_ptr=null), (0,), -1, "null"),
                                     (dict(ws_dist=3), (0,), -3, "workspace 3 <"), (dict(ws_link=64), (1,), -3, "workspace 64 <")):
        args = dict(K=33, M=8)
        args.update(kw)
        refused_dist = 0 in which
        assert (L.sq_map_row_distances_workspace_bytes(args.get("B", 1), args["K"], args["M"]) == 0) == bool(set(kw) & {"K", "M", "B"})
        codes, messages, dist, status, Z, leaves = _raw(A, **args)
        for k in which:
            assert codes[k] == code and message in messages[k], (kw, k, codes, messages)
        if refused_dist:
            assert bool((dist == SENTINEL).all()) and bool((status[0] == -7).all())
        if 1 in which:
            assert bool((Z == SENTINEL).all()) and bool((leaves == -7).all()) and bool((status[1] == -7).all())
    assert L.sq_map_linkage_average_workspace_bytes(1, 1) == 0 and L.sq_map_linkage_average_workspace_bytes(1, bound + 1) == 0
    assert L.sq_map_linkage_average_workspace_bytes(0, 5) == 0
    codes, _, dist, status, Z, leaves = _raw(A, K=33, M=8)                                  # the same helper, good arguments
    assert codes == [0, 0] and status.cpu().numpy().tolist() == [[0], [0]]
    assert Z[0, :32].cpu().numpy().tobytes() == lc.restated("rect_33x8")[1].tobytes()
    # the Python layer carries the library's message
    for K in (1, bound + 1):
        with pytest.raises(_lib.SequoiaHipArgError, match=f"K = {K} rows"):
            mapstats.linkage_average(torch.zeros(K, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.SequoiaHipArgError, match="M = 0 features"):
        mapstats.row_distances(torch.zeros(5, 0, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.SequoiaHipArgError, match="B = 0 problems"):
        mapstats.linkage_average(torch.zeros(0, 5, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        mapstats.linkage_average(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        mapstats.linkage_average(torch.zeros(5, 3, device="cuda"))
    with pytest.raises(ValueError, match="cluster_order: dtype torch.float32"):
        mapstats.cluster_order(torch.eye(5, device="cuda"))
    with pytest.raises(ValueError, match="not symmetric"):
        mapstats.cluster_order(_dev(lc.case("rect_33x8"))[:8, :8].contiguous())


def test_cluster_order_of_the_device_correlation_of_a_real_table():
    _lib.require_gpu()
    corr = mapstats.gene_correlation(_dev(lc.real_table()))
    leaves, ordered, Z = mapstats.cluster_order(corr, return_linkage=True)
    host = corr.cpu().numpy()
    _, wZ, wlv = lc.linkage(host)
    assert Z.cpu().numpy().tobytes() == wZ.tobytes() and leaves.cpu().numpy().tobytes() == wlv.tobytes()
    assert ordered.cpu().numpy().tobytes() == host[wlv][:, wlv].tobytes()
    names = [f"g{i}" for i in range(host.shape[0])]
    order, frame = mapstats.cluster_order(pd.DataFrame(host, index=names, columns=names))
    assert order.tolist() == wlv.tolist() and list(frame.index) == list(frame.columns) == [names[i] for i in wlv]
    assert frame.values.tobytes() == host[wlv][:, wlv].tobytes()


def _two_slides(root):
    """The two-slide layout of the mapstats command-line test: 70 genes, slide 2 lacks five, one NaN row each."""
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
    np.save(os.path.join(root, "ids", "all.npy"), np.array(genes[::-1][:66] + ["absent"], dtype=object))
    for k, f in enumerate(cli.CELLTYPE_FILES):
        np.save(os.path.join(root, "ids", f + ".npy"), np.array(genes[4 + 7 * k:4 + 7 * k + 9] + ["nope"], dtype=object))
    return ["--pred_folder", root, "--all_genes", os.path.join(root, "ids", "all.npy"), "--celltype_dir", os.path.join(root, "ids")]


def _listing(root):
    out = {}
    for d in cli.OUTPUT_FOLDERS:
        for f in sorted(os.listdir(os.path.join(root, d))):
            with open(os.path.join(root, d, f), "rb") as fh:
                out[os.path.join(d, f)] = fh.read()
    return out


def test_cli_clustermap_writes_the_nine_files_and_leaves_the_default_run_alone(tmp_path, capsys):
    _lib.require_gpu()
    root = str(tmp_path)
    argv = _two_slides(root)
    cli.main(argv)
    before = _listing(root)
    assert sorted(before) == ["corr_maps/s1_corr.csv", "corr_maps/s2_corr.csv", "corr_maps/total_corr.csv", "spatial_maps/s1.csv", "spatial_maps/s2.csv"]
    cli.main(argv + ["--clustermap"])
    after = _listing(root)
    new = sorted(set(after) - set(before))
    assert new == sorted(f"corr_maps/{s}_{kind}.csv" for s in ("s1", "s2", "total") for kind in ("clustered", "linkage", "order"))
    assert all(after[k] == v for k, v in before.items())                                   # the default run's files, byte for byte
    mapper = cli.gene_colors(cli.load_categories(os.path.join(root, "ids")))
    assert set(mapper.values()) == set(mapstats.COLORS.values())
    read = lambda f, **kw: pd.read_csv(os.path.join(root, "corr_maps", f), float_precision="round_trip", **kw)      # noqa: E731
    for s, K in (("s1", 66), ("s2", 61), ("total", 61)):
        corr = read(f"{s}_corr.csv", index_col=0)
        if s == "total":
            corr = corr.dropna(axis=0, how="all").dropna(axis=1, how="all")
        assert corr.shape == (K, K)
        _, wZ, wlv = lc.linkage(corr.values)
        pd.testing.assert_frame_equal(read(f"{s}_clustered.csv", index_col=0), corr.iloc[wlv, wlv], check_exact=True)
        got = read(f"{s}_linkage.csv")
        assert list(got.columns) == ["left", "right", "distance", "size"] and got.values.astype(np.float64).tobytes() == wZ.tobytes()
        order = pd.read_csv(os.path.join(root, "corr_maps", f"{s}_order.csv"), keep_default_na=False)
        genes = [corr.index[i] for i in wlv]
        assert list(order.columns) == ["gene", "color"] and order["gene"].tolist() == genes
        assert order["color"].tolist() == [mapper.get(g, "") for g in genes] and "" in order["color"].tolist()
    # a constant gene: the slide's matrix holds a NaN and is skipped by name, the others are written
    df = pd.read_csv(os.path.join(root, "s2", "stride-1.csv"))
    df["g50"] = 1.0
    df.to_csv(os.path.join(root, "s2", "stride-1.csv"), index=False)
    for f in new:
        os.remove(os.path.join(root, f))
    capsys.readouterr()
    cli.main(argv + ["--clustermap"])
    said = capsys.readouterr().out
    assert "s2: no cluster map" in said and "s1: no cluster map" not in said and "total: no cluster map" not in said
    assert sorted(set(_listing(root)) - set(before)) == [f"corr_maps/{s}_{kind}.csv" for s in ("s1", "total") for kind in ("clustered", "linkage", "order")]
    assert read("total_clustered.csv", index_col=0).shape == (60, 60)            # the constant gene's row of the mean is all NaN and dropped
