"""CPU side of the k-Means sweep (tests/kmeans_cases.py): the reference is scikit-learn's wherever scikit-learn can express
the case, every row reaches the branch it is listed for, no decision of any case is marginal, and the table notices the
mistakes it was built for.  Nothing here touches the GPU; tests/test_gpu_kmeans_sweep.py runs the same table on it.

Rows WITHOUT a scikit-learn counterpart, by design: max_iter = 0 (scikit-learn refuses it) and the exact rows
tie_farthest, all_zero, two_heaviest, dup_centres, short_of_far, strict_relocating, batch_mixed -- equal distances, equal
weights or duplicate centres, which scikit-learn orders by argpartition's internals (see kmeans_cases.py).  Their
arithmetic is exact in any order, so the oracle's rules alone decide them.

    python tests/test_kmeans_cases_host.py          rewrites profiles/kmeans_sweep_margins.txt"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import kmeans_cases as kc  # noqa: E402
from oracle import kmeans_oracle as ko  # noqa: E402

MARGINS = os.path.join(kc.ROOT, "profiles", "kmeans_sweep_margins.txt")
NO_SKLEARN = {"stop/max_iter0"} | {f"dbg/{d.name}/{s}" for d in kc.DBG_ROWS if not d.sklearn for s in range(kc.dbg_inputs(d.name)[0].shape[0])}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kmeans_sweep.npz"))


def _same_input(gold, tag, X):
    want = float(gold[tag + "::xsum"])
    assert abs(float(np.asarray(X, np.float64).sum()) - want) <= 1e-9 * max(1.0, abs(want)), tag


# ----------------------------------------------------------------------------------------------------------------------
# 1. the oracle reproduces scikit-learn
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", kc.ROWS, ids=lambda r: r.name)
def test_rows_equal_sklearn(gold, row):
    tag, ref = "row/" + row.name, kc.row_reference(row)
    _same_input(gold, tag, kc.row_data(row))
    assert np.array_equal(ref["indices"], gold[tag + "::indices"])
    assert np.array_equal(ref["labels"], gold[tag + "::labels"])
    assert ref["n_iter"] == int(gold[tag + "::n_iter"])


def test_stop_rules_and_batch_equal_sklearn(gold):
    stop = kc.ROW[kc.STOP_ROW]
    for c in kc.STOP_CASES:
        ref = kc.row_reference(stop, c.max_iter, c.tol)
        if c.max_iter == 0:
            assert "stop/" + c.name in NO_SKLEARN and ref["n_iter"] == 0
            continue
        assert np.array_equal(ref["labels"], gold[f"stop/{c.name}::labels"]) and ref["n_iter"] == int(gold[f"stop/{c.name}::n_iter"]), c.name
    b = kc.BATCH_STOP
    for s, (kind, seed) in enumerate(zip(b.kinds, b.seeds)):
        ref = kc.fit_reference(kind, seed, b.n, b.dim, b.k, b.max_iter)
        _same_input(gold, f"batch/{s}", kc.data(kind, seed, b.n, b.dim))
        assert np.array_equal(ref["indices"], gold[f"batch/{s}::indices"]) and np.array_equal(ref["labels"], gold[f"batch/{s}::labels"])
        assert ref["n_iter"] == int(gold[f"batch/{s}::n_iter"])


def test_trial_rows_seed_like_sklearn(gold):
    for t in kc.TRIAL_ROWS:
        _same_input(gold, "trial/" + t.name, kc.data(t.kind, t.seed, t.n, t.dim))
        assert np.array_equal(kc.trial_reference(t.name)["indices"], gold[f"trial/{t.name}::indices"]), t.name
    a, b = (kc.trial_reference(t.name)["indices"] for t in kc.TRIAL_ROWS)
    assert not np.array_equal(a, b)                             # the trial count matters on this data


def test_injected_centre_rows_equal_sklearn(gold):
    seen = 0
    for d in kc.DBG_ROWS:
        X, _ = kc.dbg_inputs(d.name)
        ref = kc.dbg_reference(d.name)
        for s in range(X.shape[0]):
            tag = f"dbg/{d.name}/{s}"
            if not d.sklearn:
                assert tag in NO_SKLEARN and tag + "::labels" not in gold.files
                continue
            _same_input(gold, tag, X[s])
            assert np.array_equal(ref["labels"][s], gold[tag + "::labels"]) and ref["n_iter"][s] == int(gold[tag + "::n_iter"]), tag
            seen += 1
    assert seen == 3


# ----------------------------------------------------------------------------------------------------------------------
# 2. every row reaches its branch
# ----------------------------------------------------------------------------------------------------------------------
ISSUE_ROWS = [(64, 516, 1), (500, 132, 2), (2049, 8, 3), (257, 36, 8), (1000, 252, 15), (1025, 68, 17), (400, 260, 129), (300, 4, 256),
              (256, 4, 256), (1024, 12, 100), (2048, 12, 16), (4093, 8, 255), (200, 1028, 5), (4097, 4, 3)]


def test_rows_reach_their_branch():
    assert [(r.n, r.dim, r.k) for r in kc.ROWS[:len(ISSUE_ROWS)]] == ISSUE_ROWS
    for r in kc.ROWS:
        f = kc.facts(r.n, r.dim, r.k)
        assert r.branch and r.expect
        for key, want in r.expect.items():
            assert f[key] == want, (r.name, key, f[key], want)
        assert 1 <= r.k <= kc.MAX_K and r.dim % 4 == 0 and r.k <= r.n <= kc.LARGE_MAX_N and 1 <= f["trials"] <= kc.MAX_TRIALS
    # what the older tests run at, for contrast: none of these branches
    old = kc.facts(1000, 1024, 100)
    assert old["assign_empty_groups"] == 0 and not old["gemm_k_tail"] and old["empty_slices"] == 0 and old["center_last_cols"] == 64
    assert old["lg_k_tail"] == 0 and old["norms_tail_lanes"] == 0 and old["trials"] == 6
    # the empty K slices the issue names
    assert [kc.facts(500, d, 5)["empty_slices"] for d in (260, 516, 1028, 256, 512, 1024)] == [3, 2, 1, 0, 0, 0]
    assert kc.facts(500, 252, 5)["ksl"] == 1 and kc.facts(500, 256, 5)["ksl"] == 8
    assert {kc.trials_of(k) for k in (1, 2)} == {2} and kc.trials_of(3) == 3 and kc.trials_of(100) == 6 and kc.trials_of(256) == 7
    # one ragged call spans the three seeding classes
    groups = kc.ragged_groups()
    assert any({kc.seed_class(r.n) for r in g} == {1, 2, 3} for g in groups) and all(len(g) > 1 for g in groups)
    assert sorted(t.trials for t in kc.TRIAL_ROWS) == [1, kc.MAX_TRIALS] and all(t.trials != kc.trials_of(t.k) for t in kc.TRIAL_ROWS)


def test_stop_cases_reach_their_rule():
    stop = kc.ROW[kc.STOP_ROW]
    full = kc.row_reference(stop)
    # the slowest-converging of the issue's rows, and long enough for every burst case below
    assert full["n_iter"] == max(kc.row_reference(r)["n_iter"] for r in kc.ROWS[:len(ISSUE_ROWS)]) and full["n_iter"] > 2 * kc.BURST + kc.FIRST_BURST
    ends = [kc.FIRST_BURST, kc.FIRST_BURST + kc.BURST]           # iterations after which the host polls
    by = {c.name: c for c in kc.STOP_CASES}
    assert [by[f"max_iter{m}"].max_iter for m in (0, 1, 2, 3, 6, 7)] == [0, ends[0] - 1, ends[0], ends[0] + 1, ends[1], ends[1] + 1]
    for c in kc.STOP_CASES:
        ref = kc.row_reference(stop, c.max_iter, c.tol)
        tr = ref["trace"]
        its = [r for r in tr["lloyd"] if not r["final"]]
        if c.name.startswith("max_iter"):
            assert ref["n_iter"] == c.max_iter == len(its) and not tr["strict"] and tr["lloyd"][-1]["final"]
            assert all(r["shift"] > tr["tol"] for r in its)      # stopped by max_iter and nothing else
            assert np.array_equal(ref["indices"], full["indices"])
    z = kc.row_reference(stop, 0, 1e-4)
    Xc = ko.center_data(kc.row_data(stop))[0]
    assert z["n_iter"] == 0 and np.array_equal(z["centers_c"], Xc[z["indices"]])          # centres = the seeded rows
    assert np.array_equal(z["labels"], ko._assign(Xc.astype(np.float64), Xc[z["indices"]]))
    t0 = kc.row_reference(stop, by["tol0"].max_iter, 0.0)
    assert t0["trace"]["strict"] and t0["trace"]["tol"] == 0.0 and t0["n_iter"] == full["n_iter"]
    ts = kc.row_reference(stop, by["tol_shift"].max_iter, by["tol_shift"].tol)
    its = [r for r in ts["trace"]["lloyd"] if not r["final"]]
    assert not ts["trace"]["strict"] and 2 <= ts["n_iter"] < full["n_iter"] and its[-1]["shift"] <= ts["trace"]["tol"]
    assert all(r["shift"] > ts["trace"]["tol"] for r in its[:-1]) and not np.array_equal(ts["labels"], full["labels"])
    # the batch: at least one slide converged strictly under max_iter and at least one did not
    b = kc.BATCH_STOP
    refs = [kc.fit_reference(kind, seed, b.n, b.dim, b.k, b.max_iter) for kind, seed in zip(b.kinds, b.seeds)]
    strict = [r["trace"]["strict"] for r in refs]
    assert any(strict) and not all(strict) and len(refs) == 3
    assert all(r["n_iter"] == b.max_iter for r, s in zip(refs, strict) if not s) and all(r["n_iter"] < b.max_iter for r, s in zip(refs, strict) if s)


def _iters(trace):
    return [r for r in trace["lloyd"] if not r["final"]]


def test_injected_centre_rows_reach_their_branch():
    ref = {d.name: kc.dbg_reference(d.name) for d in kc.DBG_ROWS}
    for d in kc.DBG_ROWS:                                        # exact rows: the fp32 column mean is exactly 0, Xc == X
        if not d.sklearn:
            X, _ = kc.dbg_inputs(d.name)
            for s in range(X.shape[0]):
                Xc, mean = ko.center_data(X[s])
                assert not mean.any() and np.array_equal(Xc, X[s]) and np.array_equal(X[s], np.round(X[s])), d.name
                assert sorted(map(tuple, X[s])) == sorted(map(tuple, -X[s])), d.name        # every row's negation is present
    first = lambda name, s=0: _iters(ref[name]["traces"][s])[0]      # noqa: E731
    r = first("one_empty")
    assert len(r["empty"]) == 1 and len(r["relocated"]) == 1
    r = first("three_empty")
    donors = r["labels"][r["relocated"]]
    assert len(r["empty"]) == 3 and len(r["relocated"]) == 3 and len(set(donors.tolist())) < 3
    assert kc.dbg_inputs("k1")[1].shape[1] == 1 and ref["k1"]["n_iter"][0] == 2
    r = first("tie_farthest")
    d = np.sort(r["distances"])[::-1]
    m = len(r["empty"])
    assert m == 2 and d[m - 1] == d[m] > 0                      # the cut falls inside a run of equal distances
    assert np.array_equal(r["relocated"], np.flatnonzero(r["distances"] == d[0])[:m])
    for name in ("all_zero", "two_heaviest"):
        r = first(name)
        w = r["weights"]
        assert len(r["empty"]) >= 1 and r["distances"].max() == 0 and len(r["relocated"]) == 0
        assert (w == w.max()).sum() == (1 if name == "all_zero" else 2) and r["heaviest"] == int(np.flatnonzero(w == w.max())[0])
        C = ref[name]["centers"][0]
        assert all(np.array_equal(C[e], C[r["heaviest"]]) for e in r["empty"])
        if name == "two_heaviest":
            assert not np.array_equal(C[r["empty"][0]], C[np.flatnonzero(w == w.max())[1]])
    C = kc.dbg_inputs("dup_centres")[1][0]
    r = first("dup_centres")
    assert np.array_equal(C[1], C[3]) and (r["labels"] == 3).sum() == 0 and (r["labels"] == 1).sum() > 0 and list(r["empty"]) == [3]
    r = first("short_of_far")
    assert 0 < (r["distances"] > 0).sum() < len(r["empty"]) == len(r["relocated"]) == 3
    npos = int((r["distances"] > 0).sum())
    assert np.array_equal(r["relocated"][npos:], np.flatnonzero(r["distances"] == 0)[:3 - npos])      # then distance 0, lowest index first
    tr = ref["strict_relocating"]["traces"][0]
    last = _iters(tr)[-1]
    X, _ = kc.dbg_inputs("strict_relocating")
    assert tr["strict"] and len(last["relocated"]) == 1 and np.array_equal(ref["strict_relocating"]["labels"][0], last["labels"])
    assert not np.array_equal(ko._assign(X[0].astype(np.float64), ref["strict_relocating"]["centers"][0]), last["labels"])
    bm = ref["batch_mixed"]
    assert bm["n_iter"][0] == 1 and all(bm["n_iter"][s] > 2 and len(_iters(bm["traces"][s])[1]["relocated"]) == 2 for s in (1, 2))
    assert len(_iters(bm["traces"][1])[0]["empty"]) == 0         # the clusters empty in iteration 2 were not empty in iteration 1


# ----------------------------------------------------------------------------------------------------------------------
# 3. no decision is marginal
# ----------------------------------------------------------------------------------------------------------------------
def margin_lines():
    lines = ["# tests/kmeans_cases.py: the smallest margin of every decision per case, from the oracle's trace (python "
             "tests/test_kmeans_cases_host.py).", "# pot_gap: best to runner-up potential among distinct candidates (fp64 sums, relative); "
             "round_gap: a potential's fp64 sum to the nearest fp32",
             "# rounding boundary (sums not exact in any order); cum_gap: u * pot to the neighbouring cumulative sums over pot; "
             "dist_gap: best to runner-up", "# |c|^2 - 2 x.c over |x|^2 + 2 max |c|^2 (exact rows: designed ties of 0 skipped); "
             "shift: |shift - tol| / max(shift, tol); shift_over_tol: |shift - tol| / tol.",
             f"# floor = SAFETY * m * 2^-53 with SAFETY = {kc.SAFETY:g} and m = n (pot_gap, round_gap, cum_gap), dim (dist_gap), k * dim (shift); "
             "inf: no such decision in the case."]
    worst = {}
    for tag, n, dim, k, trace, Xc, exact in kc.traced_cases():
        rec, floors = kc.margin_record(n, trace, Xc, exact), kc.margin_floors(n, dim, k)
        lines.append(f"{tag:<28} n={n:<5} dim={dim:<5} k={k:<4} " + " ".join(f"{key}={rec[key]:.3e}" for key in rec)
                     + "  floors " + " ".join(f"{key}={floors[key]:.1e}" for key in floors))
        for key, fl in floors.items():
            worst[key] = min(worst.get(key, np.inf), rec[key] / fl)
    lines.append("# smallest margin / floor over all cases: " + " ".join(f"{key}={v:.3g}" for key, v in worst.items()))
    return lines


def test_no_decision_is_marginal():
    for tag, n, dim, k, trace, Xc, exact in kc.traced_cases():
        rec, floors = kc.margin_record(n, trace, Xc, exact), kc.margin_floors(n, dim, k)
        print(tag, " ".join(f"{key}={rec[key]:.3e}" for key in rec))
        for key, fl in floors.items():
            assert rec[key] >= fl, (tag, key, rec[key], fl)
    assert kc.SAFETY >= 8 and kc.floor_sum(4096) < 2.0 ** -24 / 1000      # the floor is far below an fp32 ulp, far above an fp64 one


def test_margins_file_lists_every_case():
    text = open(MARGINS).read()
    for tag, *_ in kc.traced_cases():
        assert f"\n{tag} " in text, tag
    assert f"SAFETY = {kc.SAFETY:g}" in text


# ----------------------------------------------------------------------------------------------------------------------
# 4. the table sees the mistakes it is there for
# ----------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def _seen_by(lloyd):
    """The cases whose labels, centres or n_iter change under `lloyd`."""
    seen = []
    for d in kc.DBG_ROWS:
        a, b = kc.dbg_reference(d.name), kc.dbg_reference(d.name, lloyd)
        if _differs((a["labels"], a["centers"], a["n_iter"]), (b["labels"], b["centers"], b["n_iter"])):
            seen.append("dbg/" + d.name)
    for c in kc.STOP_CASES:
        if _differs(kc.stop_lloyd(c, ko.lloyd), kc.stop_lloyd(c, lloyd)):
            seen.append("stop/" + c.name)
    return seen


def test_unchanged_copy_of_lloyd_is_faithful():
    assert _seen_by(kc.lloyd_mutant(None)) == []


@pytest.mark.parametrize("mutant,must_see", [
    ("last_minimum", "dbg/dup_centres"), ("last_maximum", "dbg/two_heaviest"), ("ascending_relocation", "dbg/one_empty"),
    ("ties_by_higher_index", "dbg/tie_farthest"), ("no_final_e_step", "stop/max_iter3"), ("strict_not_restored", "dbg/strict_relocating"),
    ("relocation_stops_at_zero", "dbg/short_of_far")])
def test_mutant_changes_a_row(mutant, must_see):
    seen = _seen_by(kc.lloyd_mutant(mutant))
    print(mutant, "seen by", seen)
    assert must_see in seen
    assert set(kc.MUTANTS) >= {"last_minimum", "last_maximum", "ascending_relocation", "ties_by_higher_index", "no_final_e_step",
                               "strict_not_restored"}


if __name__ == "__main__":
    with open(MARGINS, "w") as f:
        f.write("\n".join(margin_lines()) + "\n")
    print("wrote", MARGINS)
