"""Host side of the ragged k-Means batch (no GPU): ragged_plan's grouping, sq_kmeans_ragged_workspace_bytes, the header."""
import os
import re

import numpy as np

from sequoia_pub_amd import _lib
from sequoia_pub_amd.kmeans import GRAM_MAX_ROWS, ragged_plan, seeding_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS_64 = [100, 257, 600, 1024, 1025, 2048, 2049, 1000]


def ws_bytes(counts, D=64, k=100):
    a = np.ascontiguousarray(counts, dtype=np.int32)
    return int(_lib.lib().sq_kmeans_ragged_workspace_bytes(len(a), a.ctypes.data if len(a) else None, D, k))


def test_plan_keeps_the_order_and_the_budget():
    rs = np.random.RandomState(3)
    counts = [int(c) for c in rs.randint(100, 4001, 40)]
    counts[7] = 5000                                          # above the Gram route: alone, through the large-slide entry
    counts[20] = 4097
    budget = 600 << 20
    plan = ragged_plan(counts, 2048, 100, budget)
    assert plan[0][0] == 0 and plan[-1][1] == len(counts)
    for (lo, hi, route), nxt in zip(plan, plan[1:] + [None]):
        assert lo < hi and (nxt is None or nxt[0] == hi)      # consecutive, in order, nothing left out
        if route == "large":
            assert hi == lo + 1 and counts[lo] > GRAM_MAX_ROWS
            continue
        assert route == "gram" and max(counts[lo:hi]) <= GRAM_MAX_ROWS
        need = ws_bytes(counts[lo:hi], 2048)
        assert 0 < need and (need <= budget or hi == lo + 1)
        if nxt is not None and nxt[2] == "gram":             # greedy: the next slide would not have fitted
            assert ws_bytes(counts[lo:hi + 1], 2048) > budget
    assert [p[:2] for p in plan if p[2] == "large"] == [(7, 8), (20, 21)]
    assert len(plan) > 4


def test_a_lone_slide_over_the_budget_still_runs_alone():
    assert ws_bytes([4000], 2048) > (64 << 20)
    assert ragged_plan([300, 4000, 300], 2048, 100, 64 << 20) == [(0, 1, "gram"), (1, 2, "gram"), (2, 3, "gram")]
    assert ragged_plan([4000], 2048, 100, 1) == [(0, 1, "gram")]


def test_plan_of_the_seeding_class_counts():
    assert ragged_plan(COUNTS_64, 64, 100, 100 << 20) == [(0, 5, "gram"), (5, 6, "gram"), (6, 8, "gram")]
    assert ragged_plan(COUNTS_64, 64, 100, 4 << 30) == [(0, 8, "gram")]
    assert ragged_plan(COUNTS_64, 64, 100, 1) == [(i, i + 1, "gram") for i in range(8)]


def test_workspace_bytes_is_zero_for_refused_shapes():
    assert ws_bytes([300, 99]) == 0                           # fewer patches than clusters
    assert ws_bytes([300, 4097]) == 0
    assert ws_bytes([300], D=62) == 0
    assert ws_bytes([300], k=257) == 0
    assert ws_bytes([]) == 0
    assert ws_bytes([100] * 4097) == 0
    assert int(_lib.lib().sq_kmeans_ragged_workspace_bytes(2, None, 64, 100)) == 0
    assert ws_bytes([100] * 4096) > 0 and ws_bytes([4096]) > 0


def test_workspace_bytes_grows_with_every_slide():
    last = 0
    for i in range(1, len(COUNTS_64) + 1):
        need = ws_bytes(COUNTS_64[:i])
        assert need > last
        last = need
    # the n x n tables dominate: 8 bytes of Gram matrix and 4 of fp32 distances per pair of patches
    assert ws_bytes([4000], 2048) > 12 * 4000 * 4000


def test_uniforms_do_not_depend_on_the_patch_count():
    """kmeans_fit_ragged hands ONE uniforms table to the call: only the first centre depends on n."""
    u0 = seeding_draws(100, 100)[1]
    for n in (101, 257, 1000, 1025, 2049, 3999, 4096):
        assert np.array_equal(seeding_draws(n, 100)[1], u0), n


def test_header_declares_the_ragged_entry():
    src = open(os.path.join(ROOT, "include", "sequoia_hip.h")).read()
    assert "kmean_features.py:65-108" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sq_kmeans_ragged_workspace_bytes", "sq_kmeans_fit_ragged"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(_lib.lib(), name)
