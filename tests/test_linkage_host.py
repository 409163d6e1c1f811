"""The numpy restatement of tests/linkage_cases.py against scipy: bit for bit on the distances, Z and the leaves of every
case in tests/golden/linkage.npz, against live scipy wherever it imports, and the bound on nearest-neighbour searches
the device kernel stops at."""
import numpy as np
import pytest

import linkage_cases as lc


@pytest.mark.parametrize("name", list(lc.CASES))
def test_restatement_equals_the_scipy_golden_bit_for_bit(name):
    g = lc.golden()
    D, Z, lv, searches = lc.restated(name)
    K = D.shape[0]
    assert Z.shape == (K - 1, 4) and lv.shape == (K,) and lv.dtype == np.int32
    assert Z.tobytes() == g[name + "_Z"].tobytes()
    assert lv.tobytes() == g[name + "_leaves"].tobytes()
    if K <= lc.GOLDEN_DIST_MAX_K:
        assert lc.condensed(D).tobytes() == g[name + "_pdist"].tobytes()
    else:
        assert lc.digest(lc.condensed(D)) == str(g[name + "_pdist_sha256"])
    assert D.tobytes() == D.T.copy().tobytes() and not D.diagonal().any()
    assert sorted(lv.tolist()) == list(range(K))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_search_count_stays_within_three_per_merge(name):
    D, _, _, searches = lc.restated(name)
    K = D.shape[0]
    print(f"{name}: {searches} searches for {K - 1} merges ({searches / (K - 1):.2f} per merge)")
    assert K - 1 <= searches <= 3 * (K - 1)


def test_ties_are_present_in_the_tie_cases():
    for name, most in (("block_48", 11), ("integers_40x6", 25), ("repeated_33x8", 33 * 16 - 30)):
        d = lc.condensed(lc.restated(name)[0])
        assert len(np.unique(d)) <= most, name
    assert int((lc.condensed(lc.restated("repeated_33x8")[0]) == 0.0).sum()) == 4          # a triple and a pair


@pytest.mark.parametrize("name", list(lc.CASES))
def test_restatement_equals_live_scipy(name):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import pdist
    A = np.array(lc.case(name))
    D, Z, lv, _ = lc.restated(name)
    assert lc.condensed(D).tobytes() == pdist(A, "euclidean").tobytes()
    want = hierarchy.linkage(A, method="average", metric="euclidean")
    assert Z.tobytes() == want.tobytes()
    assert lv.tolist() == hierarchy.leaves_list(want).tolist() == hierarchy.dendrogram(want, no_plot=True)["leaves"]


def test_first_nonfinite_row_and_a_nan_gene():
    c = np.array(lc.case("corr_17"))
    c[5, :] = np.nan
    c[:, 5] = np.nan
    assert lc.first_nonfinite_row(lc.row_distances(c)) == 0              # the NaN column is a feature of every row
    assert lc.first_nonfinite_row(lc.restated("corr_17")[0]) == -1
