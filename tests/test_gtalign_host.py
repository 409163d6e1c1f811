"""What the device ground-truth alignment can be held to without a GPU: the numpy restatement of tests/gtalign_cases.py
equals the reference's literal get_average, median_filter, score2percentile and np.unique on every golden case
(tests/golden/gtalign.npz) bit for bit, every constructed case has the property it is named for, and the argument refusals
that need no device: the library's checks run before its first launch."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gtalign_cases as gc
from sequoia_pub_amd import _lib, gtalign


def _crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(gc.bits(got), gc.bits(want))


def test_golden_inputs_are_the_ones_the_file_was_made_from():
    g = gc.golden()
    for name, c in gc.nearest_cases().items():
        assert _crc(*c[:4]) == int(g[f"ns_{name}_crc"][0]), name
    for dtype in ("float32", "float64"):
        assert _crc(*gc.means_case(dtype)) == int(g[f"means_{dtype}_crc"][0]), dtype
    for name, c in gc.median_cases().items():
        assert _crc(*c) == int(g[f"mf_{name}_crc"][0]), name
    for name, v in gc.unique_cases().items():
        assert _crc(v) == int(g[f"uq_{name}_crc"][0]), name
    assert _crc(*gc.whole_case().values()) == int(g["whole_crc"][0])
    assert gtalign.spot_chunk() == gc.SPOT_CHUNK and gtalign.unique_chunk_rows() == gc.UNIQUE_CHUNK


@pytest.mark.parametrize("name", list(gc.nearest_cases()))
def test_restated_nearest_spots_equal_the_literal_sort(name):
    xc, yc, sx, sy, k = gc.nearest_cases()[name]
    idx, dist = gc.nearest(xc, yc, sx, sy, k)
    assert idx.shape == (len(xc), min(k, len(sx))) and _same(idx, gc.golden()[f"ns_{name}_idx"])
    assert np.all(np.diff(dist, axis=1) >= 0)


def test_lattice_tiles_have_exact_ties_that_the_stable_order_decides():
    xc, yc, sx, sy, _ = gc.nearest_cases()["ties_k8"]
    d = np.sort(gc.distances(xc, yc, sx, sy)[gc.LATTICE_INTERIOR], axis=1)
    assert len(sx) == 37 and len(gc.LATTICE_INTERIOR) == 9
    assert np.all(d[:, 0] == d[:, 3]) and np.all(d[:, 3] < d[:, 4]) and np.all(d[:, 4] == d[:, 11]) and np.all(d[:, 11] < d[:, 12])
    for k in (1, 4, 8):                                     # the cut falls inside a tie: the kept spots are the lower indices
        idx = gc.golden()[f"ns_ties_k{k}_idx"][gc.LATTICE_INTERIOR]
        ring = np.argsort(gc.distances(xc, yc, sx, sy)[gc.LATTICE_INTERIOR], axis=1, kind="stable")
        first = ring[:, :4] if k <= 4 else ring[:, 4:12]
        kept = idx[:, :k] if k <= 4 else idx[:, 4:]
        assert np.array_equal(kept, np.sort(first, axis=1)[:, :kept.shape[1]])
    assert not np.array_equal(np.sort(sx), sx)              # the index order is no lattice order


def test_sqrt_collapse_pair_is_decided_on_d_not_on_d_squared():
    xc, yc, sx, sy, k, attempt = gc.sqrt_collapse_pair()
    dx, dy = sx - xc[0], sy - yc[0]
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2)
    assert d2[0] == np.nextafter(d2[1], np.inf) and d[0] == d[1]              # one ulp apart, the larger first, one d
    by_d, by_d2 = np.argsort(d, kind="stable"), np.argsort(d2, kind="stable")
    assert by_d[k - 1] == 0 and by_d[k] == 1 and by_d2[k - 1] == 1 and by_d2[k] == 0          # positions k and k + 1
    assert gc.golden()["ns_sqrt_collapse_idx"][0, k - 1] == 0
    print(f"sqrt-collapse pair found at candidate {attempt}")


def test_contraction_case_orders_the_pair_differently_when_fused():
    tx, ty, p, q, attempt = gc.contraction_pair()
    u, v = gc.fma_d2(p, q), gc.fma_d2(q, p)
    assert p * p + q * q == q * q + p * p and u != v and np.sqrt(u) != np.sqrt(v)
    wrong = 0
    for name, first in (("contraction_ab", (p, q)), ("contraction_ba", (q, p))):
        xc, yc, sx, sy, k = gc.nearest_cases()[name]
        assert k == 1 and sx[0] - xc[0] == first[0] and sy[0] - yc[0] == first[1] and sx[1] - xc[0] == first[1] and sy[1] - yc[0] == first[0]
        assert gc.golden()[f"ns_{name}_idx"].tolist() == [[0]]                  # separately rounded: a tie, the lower index
        for fused in (lambda a, b: gc.fma_d2(a, b), lambda a, b: gc.fma_d2(b, a)):          # the two shapes of the contraction
            wrong += int(fused(*first) > fused(first[1], first[0]))
    assert wrong == 2                                        # each shape picks index 1 in one of the two orders
    print(f"contraction case found at candidate {attempt}")


def test_chunk_cases_keep_spots_of_the_last_partial_chunk_and_across_a_border():
    for n_spots in (gc.SPOT_CHUNK - 1, gc.SPOT_CHUNK, gc.SPOT_CHUNK + 1, 2 * gc.SPOT_CHUNK + 3):
        idx = gc.golden()[f"ns_chunk_{n_spots}_idx"]
        near = gc.chunk_near_indices(n_spots)
        assert 2 <= len(near) <= 4 and all(set(near) <= set(row) for row in idx.tolist())       # every tile keeps the placed neighbours
        assert (idx == n_spots - 1).any()
        if n_spots > gc.SPOT_CHUNK:
            border = (n_spots - 1) // gc.SPOT_CHUNK * gc.SPOT_CHUNK
            assert (idx == border).any() and (idx == border - 1).any()
    assert gc.golden()["ns_spots_1_idx"].shape == (7, 1) and gc.golden()["ns_spots_3_idx"].shape == (7, 3)
    assert (gc.nearest_cases()["negative"][2] < 0).any() and gc.nearest_cases()["near_1e5"][2].min() > 9.9e4


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_restated_means_equal_np_mean_of_the_kept_values(dtype):
    xc, yc, sx, sy, expr = gc.means_case(dtype)
    g = gc.golden()
    assert expr.dtype == np.dtype(dtype) and expr.shape[1] > len(gc.MEANS_COLS)
    for k in gc.MEANS_KS:
        idx, _ = gc.nearest(xc, yc, sx, sy, k)
        got, want = gc.spot_means(idx, expr, gc.MEANS_COLS), g[f"means_{dtype}_k{k}"]
        assert _same(got, want), k
        rot = gc.spot_means(np.roll(idx, 1, axis=1), expr, gc.MEANS_COLS)
        # f64: the rotated sum differs somewhere, so the order of the adds shows (sums of a few f32 values are exact in f64)
        assert int((gc.bits(rot) != gc.bits(got)).sum()) > 0 or dtype == "float32"
    want = g[f"means_{dtype}_k3"]
    assert np.isnan(want[0, 0]) and np.isnan(want[0, 1]) and np.isfinite(want[0, 2])          # the NaN member; inf + -inf
    eight = g[f"means_{dtype}_k8"][-1, 2]
    assert eight == 0.0 and not np.signbit(eight)


def test_the_mean_of_eight_is_numpys_pairwise_block_not_the_sequential_sum():
    xc, yc, sx, sy, expr = gc.means_case("float64")
    idx, _ = gc.nearest(xc, yc, sx, sy, 8)
    e = expr[:, gc.MEANS_COLS]
    seq = np.zeros((len(xc), len(gc.MEANS_COLS)))
    with np.errstate(all="ignore"):
        for j in range(8):
            seq = seq + e[idx[:, j]]
    want = gc.golden()["means_float64_k8"]
    assert int((gc.bits(seq / 8.0) != gc.bits(want)).sum()) > 0


@pytest.mark.parametrize("name", list(gc.median_cases()))
def test_restated_median_filter_equals_the_literal_function(name):
    values, xtf, ytf = gc.median_cases()[name]
    for r in gc.MEDIAN_RADII:
        for na in (0, 1):
            got, _ = gc.median_filter(values, xtf, ytf, r, bool(na))
            assert _same(got, gc.golden()[f"mf_{name}_r{r}_na{na}"]), (r, na)


def test_median_cases_have_the_counts_and_values_they_are_named_for():
    c = gc.median_cases()
    values, xtf, ytf = c["sparse"]
    assert not np.array_equal(np.lexsort((ytf, xtf)), np.arange(len(xtf)))                    # rows in permuted order
    assert len(set(zip(xtf.tolist(), ytf.tolist()))) == len(xtf)
    nan_rows = [set(np.flatnonzero(np.isnan(values[:, k])).tolist()) for k in range(3)]
    assert nan_rows[0] and nan_rows[1] and not nan_rows[2] and nan_rows[0] != nan_rows[1]
    for r, edge in ((1, (4, 5)), (2, (12, 13)), (3, (24, 25))):
        for na in (False, True):
            _, counts = gc.median_filter(values, xtf, ytf, r, na)
            seen = set(counts[:, 2].tolist())
            assert set(edge) <= seen, (r, sorted(seen))
            if r == 1:
                assert {6, 8} <= seen and {7, 9} <= seen                                       # even and odd medians
    out0, out1 = gc.median_filter(values, xtf, ytf, 1, False)[0], gc.median_filter(values, xtf, ytf, 1, True)[0]
    clean = ~np.isnan(values[:, 0])
    assert np.isnan(out0[clean, 0]).any() and not np.isnan(out1[clean, 0]).any() and np.isnan(out1[~clean, 0]).all()
    _, counts = gc.median_filter(*c["full"], 1, False)
    assert sorted(set(counts[:, 0].tolist())) == [4, 6, 9]
    got, counts = gc.median_filter(*c["line"], 1, False)
    assert counts.max() == 3 and _same(got, np.array(c["line"][0]))                          # every row keeps its own value
    got, counts = gc.median_filter(*c["one"], 3, False)
    assert counts.tolist() == [[1]] and got.tolist() == [[2.5]]
    g = gc.golden()
    mid = lambda name: g[f"mf_six_{name}_r1_na0"][c["six_" + name][1] == 1, 0]               # noqa: E731  the middle column's rows
    assert np.all(mid("zeros") == 0.0) and not np.signbit(mid("zeros")).any() and not np.signbit(mid("neg_zeros")).any()
    assert np.all(mid("inf_inf") == np.inf) and np.isnan(mid("minf_inf")).all() and np.all(mid("overflow") == np.inf)
    assert np.isnan(mid("nan")).all() and np.all(g["mf_six_nan_r1_na1"][(c["six_nan"][1] == 1) & ~np.isnan(c["six_nan"][0][:, 0]), 0] == 4.0)
    centre = (c["nine_neg_zero"][1] == 1) & (c["nine_neg_zero"][2] == 1)
    nine = g["mf_nine_neg_zero_r1_na0"][centre, 0]
    assert nine[0] == 0.0 and not np.signbit(nine[0]) and np.signbit(c["nine_neg_zero"][0][:, 0]).sum() == 6


@pytest.mark.parametrize("name", list(gc.unique_cases()))
def test_restated_unique_counts_equal_np_unique(name):
    v = gc.unique_cases()[name]
    assert int(gc.count_unique(v)[0]) == int(gc.golden()[f"uq_{name}"][0])


def test_unique_cases_have_their_properties():
    u = gc.unique_cases()
    g = gc.golden()
    assert int(g["uq_specials"][0]) == 3 and int(g["uq_one"][0]) == 1 and int(g["uq_equal"][0]) == 1 and int(g["uq_distinct"][0]) == 1000
    b = u["border"]
    assert len(b) > gc.UNIQUE_CHUNK and set(b[gc.UNIQUE_CHUNK:].tolist()) <= set(b[:gc.UNIQUE_CHUNK].tolist())       # nothing new behind the border
    assert b[gc.UNIQUE_CHUNK - 1] == b[gc.UNIQUE_CHUNK] and int(g["uq_border"][0]) == 41
    assert len(u["many"]) > 2 * gc.UNIQUE_CHUNK and np.isnan(u["many"]).sum() == 3 and int(g["uq_all_nan"][0]) == 1


def test_restated_chain_equals_the_literal_chain():
    g = gc.golden()
    rows, per_gene = gc.whole_restated()
    assert len(rows) == 59 and gc.WHOLE_NAN_ROW not in rows
    lost = 0
    for gene, r in per_gene.items():
        assert np.array_equal(rows[r["sub"]], g[f"whole_{gene}_rows"]), gene
        assert _same(r["ground_truth"], g[f"whole_{gene}_ground_truth"]), gene
        assert _same(r["ground_truth_filt"], g[f"whole_{gene}_ground_truth_filt"]), gene
        assert _same(r["pred_filt"], g[f"whole_{gene}_filt"]), gene
        assert [r["nr_gt_vals"], r["nr_gt_vals_filt"]] == g[f"whole_{gene}_nr"].tolist(), gene
        lost += len(rows) - len(r["sub"])
    assert lost >= 1 and len(per_gene[gc.WHOLE_GENES[1]]["sub"]) < 59 and len(per_gene[gc.WHOLE_GENES[0]]["sub"]) == 59


def test_library_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                # never followed: every refusal precedes the first launch
    mr = gtalign.MAX_ROWS

    def ns(n_tiles=5, n_spots=9, k=4, xc=one):
        return L.sq_gt_nearest_spots(xc, one, n_tiles, one, one, n_spots, k, one, null, null)

    def sm(n_tiles=5, k_eff=4, n_spots=9, ld=3, C=3, f64=0, expr=one):
        return L.sq_gt_spot_means(one, n_tiles, k_eff, expr, f64, n_spots, ld, null, C, one, null)

    def mf(n=5, ld=2, C=2, gw=3, gh=3, r=1, na=0, flag=one, ws_bytes=1 << 20):
        return L.sq_gt_median_filter(one, n, ld, null, C, one, one, gw, gh, r, na, one, null, flag, one, ws_bytes, null)

    def uq(n=5, ld=2, C=2, ws_bytes=1 << 30):
        return L.sq_gt_count_unique(one, n, ld, null, C, one, one, ws_bytes, null)

    for call, code, message in ((lambda: ns(n_tiles=0), -1, "n_tiles = 0"), (lambda: ns(n_tiles=mr + 1), -1, f"n_tiles = {mr + 1}"),
                                (lambda: ns(n_spots=0), -1, "n_spots = 0"), (lambda: ns(n_spots=(1 << 20) + 1), -1, "n_spots = 1048577"),
                                (lambda: ns(k=0), -1, "k = 0"), (lambda: ns(k=9), -1, "k = 9"), (lambda: ns(xc=null), -1, "null"),
                                (lambda: ns(xc=ctypes.c_void_p(12)), -1, "misaligned"),
                                (lambda: sm(n_tiles=0), -1, "n_tiles = 0"), (lambda: sm(k_eff=0), -1, "k_eff = 0"), (lambda: sm(k_eff=9), -1, "k_eff = 9"),
                                (lambda: sm(k_eff=4, n_spots=3), -1, "k_eff = 4"), (lambda: sm(C=0), -1, "C = 0"), (lambda: sm(C=4), -1, "C <= ld"),
                                (lambda: sm(f64=2), -1, "expr_f64 = 2"), (lambda: sm(expr=null), -1, "null"),
                                (lambda: mf(n=0), -1, "n = 0 rows"), (lambda: mf(n=mr + 1), -1, f"n = {mr + 1} rows"), (lambda: mf(C=3), -1, "C <= ld"),
                                (lambda: mf(gw=0), -1, "grid 0 x 3"), (lambda: mf(gw=4097, gh=4096), -1, "grid 4097 x 4096"),
                                (lambda: mf(r=0), -1, "r = 0"), (lambda: mf(r=4), -1, "r = 4"), (lambda: mf(na=2), -1, "nan_absent = 2"),
                                (lambda: mf(flag=null), -1, "null"), (lambda: mf(gw=100, gh=100, ws_bytes=1024), -3, "workspace 1024 <"),
                                (lambda: uq(n=0), -1, "n = 0 rows"), (lambda: uq(n=mr + 1), -1, f"n = {mr + 1} rows"), (lambda: uq(C=0), -1, "C = 0"),
                                (lambda: uq(C=65537), -1, "C = 65537"), (lambda: uq(C=3), -1, "C <= ld"), (lambda: uq(ws_bytes=64), -3, "workspace 64 <")):
        assert call() == code and message in L.sq_last_error().decode(), (message, L.sq_last_error())
    # the size functions are host arithmetic: 0 for every refused shape
    assert L.sq_gt_median_filter_workspace_bytes(0, 3, 3) == 0 and L.sq_gt_median_filter_workspace_bytes(5, 0, 3) == 0
    assert L.sq_gt_median_filter_workspace_bytes(5, 4097, 4096) == 0 and L.sq_gt_median_filter_workspace_bytes(mr + 1, 3, 3) == 0
    assert L.sq_gt_median_filter_workspace_bytes(5, 4096, 4096) == 4 << 24 and L.sq_gt_median_filter_workspace_bytes(1, 1, 1) >= 4
    assert L.sq_gt_count_unique_workspace_bytes(0, 1) == 0 and L.sq_gt_count_unique_workspace_bytes(mr + 1, 1) == 0
    assert L.sq_gt_count_unique_workspace_bytes(5, 0) == 0 and L.sq_gt_count_unique_workspace_bytes(5, 65537) == 0
    assert L.sq_gt_count_unique_workspace_bytes(gc.UNIQUE_CHUNK + 1, 3) >= 3 * 2 * gc.UNIQUE_CHUNK * 8


def test_python_layer_checks_arguments_and_never_falls_back():
    x = torch.zeros(6, dtype=torch.float64)
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="num_tiles"):
            gtalign.nearest_spots(x, x, x, x, num_tiles=bad)
    with pytest.raises(ValueError, match="differ in shape"):
        gtalign.nearest_spots(x, x[:5], x, x)
    with pytest.raises(ValueError, match="int32"):
        gtalign.spot_means(torch.zeros(3, 4, dtype=torch.int64), torch.zeros(9, 2))
    with pytest.raises(ValueError, match="no columns of the prediction table"):
        gtalign.align_ground_truth(torch.zeros(4, 2), ["a", "b"], x[:4], x[:4], x[:4], x[:4], x, x, torch.zeros(6, 1), ["c"])
    with pytest.raises(ValueError, match="one column per requested gene"):
        gtalign.align_ground_truth(torch.zeros(4, 2), ["a", "b"], x[:4], x[:4], x[:4], x[:4], x, x, torch.zeros(6, 2), ["a"])
    if not torch.cuda.is_available():
        idx = torch.zeros(3, 4, dtype=torch.int32)
        for call in (lambda: gtalign.nearest_spots(x, x, x, x), lambda: gtalign.spot_means(idx, torch.zeros(9, 2)),
                     lambda: gtalign.median_filter(x, torch.arange(6), torch.arange(6)), lambda: gtalign.count_unique(x)):
            with pytest.raises(_lib.SequoiaHipError):
                call()
