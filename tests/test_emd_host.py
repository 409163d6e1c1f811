"""What the device earth mover's distance can be held to without a GPU: the numpy restatement of tests/emd_cases.py (fill,
shift, normalise, shortest augmenting paths) reaches linprog's optimum in tests/golden/emd.npz on every case and its own
plan passes the certificate; the certificate check rejects a plan that is not one; every ``sq_emd_*`` symbol of the header
has a registered signature; and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import emd_cases as ec
from sequoia_pub_amd import _abi, _lib, emd

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sequoia_hip.h")


def _restated(arr0, arr1, label):
    """The restatement's value for one pair of grids; where there is a problem to solve, its certificate is checked."""
    s0, s1 = ec.signature(arr0), ec.signature(arr1)
    value = ec.emd(arr0, arr1)
    if s0 is not None and s1 is not None:
        got, u, v, ij, f, stats = ec.solve(s0[1], s0[0], s1[1], s1[0])
        assert got == value
        ec.check_certificate(s0[1], s1[1], (s0[0], s1[0]), u, v, (ij, f), got, label=f"restatement {label}")
        print(f"restatement {label}: {stats['augmentations']} augmentations, {stats['steps']} search steps, {len(f)} arcs")
    return value


def test_golden_inputs_are_the_ones_the_file_was_made_from():
    g = ec.golden()
    for name, case in ec.cases().items():
        assert ec.case_crc(case) == int(g[name + "_crc"][0]), name
    assert ec.crc(*ec.batch_case()) == int(g["batch_crc"][0]) and ec.crc(*ec.table_case()) == int(g["table_crc"][0])
    assert len(g["batch_values"]) == len(ec.BATCH_CELLS) >= 16 and len(g["table_values"]) == len(ec.TABLE_COLS_A)
    arr0, arr1 = ec.limit_case()
    assert ec.crc(arr0, arr1) == int(g["limit_crc"][0]) and arr0.shape == ec.LIMIT_SHAPE
    assert all(len(ec.signature(a)[1]) == ec.MAX_CELLS for a in (arr0, arr1)) and 10 <= int((arr0 != arr1).sum()) <= 24


@pytest.mark.parametrize("name", list(ec.cases()))
def test_restatement_equals_the_golden(name):
    want = float(ec.golden()[name + "_value"][0])
    got = _restated(*ec.grids_of(ec.cases()[name]), name)
    print(f"{name}: restatement {got!r}, linprog {want!r}")
    assert ec.close_to_golden(got, want)


def test_restatement_equals_the_golden_on_the_batch_and_the_table():
    g = ec.golden()
    for p, (a, b) in enumerate(zip(*ec.batch_case())):
        assert ec.close_to_golden(_restated(a, b, f"batch {p}"), float(g["batch_values"][p])), p
    a, b, xtf, ytf = ec.table_case()
    for p, (ja, jb) in enumerate(zip(ec.TABLE_COLS_A, ec.TABLE_COLS_B)):
        assert ec.close_to_golden(_restated(*ec.fill_shift(a[:, ja], b[:, jb], xtf, ytf), f"table {p}"), float(g["table_values"][p])), p


def test_cases_have_the_properties_they_are_named_for():
    c, g = ec.cases(), ec.golden()
    count = lambda name: tuple(len(s[1]) for s in map(ec.signature, ec.grids_of(c[name])))      # noqa: E731
    assert count("single") == (1, 1) and count("one_to_many") == (1, 7) and count("many_to_one") == (5, 1)
    assert float(g["single_value"][0]) == np.sqrt(8.0) and float(g["identical_value"][0]) == 0.0 and float(g["both_zero_value"][0]) == 0.0
    assert np.isnan(g["first_zero_value"][0]) and np.isnan(g["second_zero_value"][0])
    n, m = count("n_ne_m")
    assert n != m
    for name, (h, w) in (("perc_6x7", (6, 7)), ("perc_12x13", (12, 13)), ("raw_6x7", (6, 7)), ("raw_12x13", (12, 13))):
        case = c[name]
        arr0, arr1 = ec.grids_of(case)
        assert arr0.shape == (h, w) and 0.75 <= len(case["a"]) / (h * w) <= 0.85
        if name.startswith("raw"):                           # the shift makes every empty cell positive
            assert case["a"].min() < 0 and case["b"].min() < 0 and count(name) == (h * w - 1, h * w - 1)
        else:                                                # ties within a map and weights shared between the maps: degenerate
            assert len(np.unique(case["a"])) < len(case["a"]) and len(np.unique(case["b"])) < len(case["b"])
            assert len(set(case["a"].tolist()) & set(case["b"].tolist())) >= 5                 # weights both maps hold
    full = c["full_positive"]
    arr0, arr1 = ec.grids_of(full)
    assert full["a"].min() > 0 and len(full["a"]) == arr0.size and arr0.min() == 2 * full["a"].min() and count("full_positive") == (20, 20)
    n, m = count("chunk")
    assert n <= 40 and m == ec.COLUMN_CHUNK + 1
    a, b, xtf, ytf = ec.table_case()
    whole = ec.fill_shift(a[:, 0], b[:, 1], xtf, ytf)[0].shape
    shrunk = ec.fill_shift(a[:, ec.TABLE_COLS_A[ec.TABLE_NAN_PROBLEM]], b[:, ec.TABLE_COLS_B[ec.TABLE_NAN_PROBLEM]], xtf, ytf)[0].shape
    assert whole == (6, 7) and shrunk == (5, 6)
    sizes = {tuple(len(s[1]) if s is not None else 0 for s in map(ec.signature, pair)) for pair in zip(*ec.batch_case())}
    assert len(sizes) >= 16 and (0, 0) in sizes


def test_certificate_check_rejects_a_perturbed_plan():
    (ca, wa), (cb, wb) = map(ec.signature, ec.grids_of(ec.cases()["raw_6x7"]))
    value, u, v, ij, f, _ = ec.solve(wa, ca, wb, cb)
    ec.check_certificate(wa, wb, (ca, cb), u, v, (ij, f), value)
    bent = f.copy()
    bent[3] += 1e-9                                           # one arc perturbed: the marginals no longer hold
    with pytest.raises(AssertionError):
        ec.check_certificate(wa, wb, (ca, cb), u, v, (ij, bent), value)
    for duals in ((np.concatenate([u[:2], u[2:3] + 1e-6, u[3:]]), v), (u, np.concatenate([v[:5], v[5:6] + 1e-6, v[6:]]))):
        with pytest.raises(AssertionError):                  # duals shifted up on one node: infeasible
            ec.check_certificate(wa, wb, (ca, cb), duals[0], duals[1], (ij, f), value)
    with pytest.raises(AssertionError):                      # shifted down: feasible, but the objectives part
        ec.check_certificate(wa, wb, (ca, cb), np.concatenate([u[:2], u[2:3] - 1e-6, u[3:]]), v, (ij, f), value)
    with pytest.raises(AssertionError):
        ec.check_certificate(wa, wb, (ca, cb), u, v, (ij, f), value + 1e-9)
    with pytest.raises(AssertionError):                      # a feasible flow that is not optimal
        rows, cols = np.arange(len(wa)), np.arange(len(wb))
        ec.check_certificate(wa, wb, (ca, cb), u, v, (np.stack(np.meshgrid(rows, cols, indexing="ij"), -1).reshape(-1, 2), np.outer(wa, wb).ravel()),
                             float(np.sum(np.outer(wa, wb) * ec.cost_matrix(ca, cb))))


def test_restatement_reports_its_augmentation_cap():
    (ca, wa), (cb, wb) = map(ec.signature, ec.grids_of(ec.cases()["raw_6x7"]))
    with pytest.raises(ec.AugmentationCap):
        ec.solve(wa, ca, wb, cb, max_augmentations=1)


def test_every_emd_symbol_of_the_header_has_a_registered_signature():
    text = open(HEADER).read()
    symbols = sorted(set(re.findall(r"\b(sq_emd_\w+)\s*\(", text)))
    assert len(symbols) >= 7 and {"sq_emd_fill", "sq_emd_solve", "sq_emd_workspace_bytes", "sq_emd_column_chunk"} <= set(symbols)
    L = _lib.lib()
    for s in symbols:
        assert s in _abi.FUNCTIONS, s
        assert hasattr(L, s), s
        assert getattr(L, s).restype == _abi.FUNCTIONS[s][0] and getattr(L, s).argtypes == _abi.FUNCTIONS[s][1], s
    limits = dict(re.findall(r"#define (SQ_EMD_MAX_\w+) (\d+)", text))
    assert int(limits["SQ_EMD_MAX_CELLS"]) == emd.MAX_CELLS == ec.MAX_CELLS >= 4096 and int(limits["SQ_EMD_MAX_DIM"]) == emd.MAX_DIM
    assert int(limits["SQ_EMD_MAX_GRID_CELLS"]) == emd.MAX_GRID_CELLS and int(limits["SQ_EMD_MAX_PROBLEMS"]) == emd.MAX_PROBLEMS
    assert int(limits["SQ_EMD_MAX_ARCS"]) == emd.MAX_ARCS
    assert int(re.search(r"#define SQ_EMD_DEFAULT_AUGMENTATIONS (\d+)", text).group(1)) == emd.DEFAULT_AUGMENTATIONS == ec.DEFAULT_AUGMENTATIONS
    assert emd.column_chunk() == ec.COLUMN_CHUNK
    assert "get_emd.py:54-90,180-189" in text


def test_library_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)     # never followed: every refusal precedes the first launch

    def fill(n=5, P=2, lda=2, ldb=2, gh=3, gw=3, cells=9, na=1, a=one, ws_bytes=1 << 20):
        return L.sq_emd_fill(a, lda, null, one, ldb, null, n, one, one, P, na, gh, gw, cells, one, one, one, one, ws_bytes, null)

    def solve(cells=9, P=2, cap=4, arcs=64, max_aug=0, grids=one, ws_bytes=1 << 30):
        return L.sq_emd_solve(grids, cells, one, P, cap, arcs, max_aug, *([one] * 12), one, ws_bytes, null)

    for call, code, message in ((lambda: fill(n=0), -1, "n = 0 rows"), (lambda: fill(P=0), -1, "P = 0"), (lambda: fill(P=65537), -1, "P = 65537"),
                                (lambda: fill(P=3), -1, "P <= ld"), (lambda: fill(gh=0), -1, "grid 0 x 3"), (lambda: fill(gh=16385, cells=1 << 24), -1, "grid 16385 x 3"),
                                (lambda: fill(cells=8), -1, "cells = 8"), (lambda: fill(na=2), -1, "nan_absent = 2"), (lambda: fill(a=null), -1, "null"),
                                (lambda: fill(a=ctypes.c_void_p(12)), -1, "misaligned"), (lambda: fill(cells=4096, ws_bytes=64), -3, "workspace 64 <"),
                                (lambda: solve(P=0), -1, "P = 0"), (lambda: solve(cells=0), -1, "cells = 0"), (lambda: solve(cap=0), -1, "cap_cells = 0"),
                                (lambda: solve(cap=4097), -1, "cap_cells = 4097"), (lambda: solve(arcs=0), -1, "arc_cap = 0"),
                                (lambda: solve(arcs=16385), -1, "arc_cap = 16385"), (lambda: solve(max_aug=-1), -1, "max_aug = -1"),
                                (lambda: solve(grids=null), -1, "null"), (lambda: solve(ws_bytes=64), -3, "workspace 64 <")):
        assert call() == code and message in L.sq_last_error().decode(), (message, L.sq_last_error())
    # the size functions are host arithmetic: 0 exactly for the refused shapes
    assert L.sq_emd_workspace_bytes(0, 4, 64) == 0 and L.sq_emd_workspace_bytes(2, 0, 64) == 0 and L.sq_emd_workspace_bytes(2, 4097, 64) == 0
    assert L.sq_emd_workspace_bytes(2, 4, 0) == 0 and L.sq_emd_workspace_bytes(2, 4, 16385) == 0 and L.sq_emd_workspace_bytes(65537, 4, 64) == 0
    assert L.sq_emd_workspace_bytes(1, 1, 1) > 0 and L.sq_emd_workspace_bytes(128, 4096, 16384) >= 128 * (4096 * 28 + 16384 * 4)
    assert L.sq_emd_fill_workspace_bytes(0, 9) == 0 and L.sq_emd_fill_workspace_bytes(2, 0) == 0 and L.sq_emd_fill_workspace_bytes(2, (1 << 24) + 1) == 0
    assert L.sq_emd_fill_workspace_bytes(2, 9) >= 72
    # a status that is not OK becomes the library's error text, naming the problem
    status = (ctypes.c_int32 * 3)(0, 0, 2)
    assert L.sq_emd_status_check(ctypes.cast(status, ctypes.c_void_p), 3) == -4 and "problem 2" in L.sq_last_error().decode()
    assert "augmentations" in L.sq_last_error().decode() and L.sq_emd_status_check(ctypes.cast(status, ctypes.c_void_p), 2) == 0
    assert b"arc" in L.sq_emd_status_text(3)


def test_python_layer_checks_arguments_and_never_falls_back():
    g = torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="one shape"):
        emd.emd_grids(g, g[:2])
    with pytest.raises(ValueError, match="one shape"):
        emd.emd_grids(g[0], g[0])
    with pytest.raises(ValueError, match="float64"):
        emd.emd_grids(g.float(), g.float())
    with pytest.raises(TypeError):
        emd.emd_grids(g.numpy(), g.numpy())
    with pytest.raises(ValueError, match="grid 16385 x 1"):
        emd.emd_grids(torch.zeros(16385, 1, dtype=torch.float64), torch.zeros(16385, 1, dtype=torch.float64))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_augmentations"):
            emd.emd_grids(g, g, max_augmentations=bad)
        with pytest.raises(ValueError, match="max_augmentations"):
            emd.emd_maps(g, g, torch.arange(3), torch.arange(3), max_augmentations=bad)
    if not torch.cuda.is_available():
        for call in (lambda: emd.emd_grids(g, g), lambda: emd.emd_maps(g, g, torch.arange(3), torch.arange(3))):
            with pytest.raises(_lib.SequoiaHipError):
                call()
