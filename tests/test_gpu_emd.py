"""sequoia_pub_amd.emd (csrc/emd.hip) on the device: every value against linprog's optimum in tests/golden/emd.npz (1e-9
relative; the restatement of tests/emd_cases.py reached it on the host), the optimality certificate on every returned plan
(emd_cases.check_certificate: a feasible flow and feasible duals of equal objective prove the optimum without trusting any
solver), two calls giving the same bytes, the conventions, the refusals, the bounded-work exit, and the two columns in
``align_ground_truth(emd=True)`` and ``cli.get_emd --emd``."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import emd_cases as ec  # noqa: E402
import gtalign_cases as gc  # noqa: E402
from sequoia_pub_amd import _lib, emd, gtalign  # noqa: E402
from sequoia_pub_amd.cli import get_emd as cli  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _host(plan):
    out = {k: v.cpu().numpy() for k, v in plan.items() if torch.is_tensor(v)}
    out["arcs"] = (plan["arcs"][0].cpu().numpy(), plan["arcs"][1].cpu().numpy())
    return out


def _plan_bytes(values, plans):
    parts = [values.cpu().numpy().tobytes()]
    for plan in plans:
        h = _host(plan)
        parts += [h[k].tobytes() for k in ("coords_a", "w_a", "coords_b", "w_b", "u", "v")] + [h["arcs"][0].tobytes(), h["arcs"][1].tobytes()]
    return b"".join(parts)


def _check_plan(plan, arr0, arr1, value, label):
    """The plan is over the restatement's own signatures (same cells, same weights to the last bit or two) and certifies."""
    h = _host(plan)
    s0, s1 = ec.signature(arr0), ec.signature(arr1)
    if s0 is None or s1 is None:
        assert len(h["w_a"]) == 0 and len(h["w_b"]) == 0 and len(h["arcs"][1]) == 0
        return
    assert np.array_equal(h["coords_a"], s0[0]) and np.array_equal(h["coords_b"], s1[0]), label
    assert np.abs(h["w_a"] - s0[1]).max() <= 4e-16 and np.abs(h["w_b"] - s1[1]).max() <= 4e-16, label       # the sum's order: a few ulp of a weight <= 1
    ec.check_certificate(h["w_a"], h["w_b"], (h["coords_a"], h["coords_b"]), h["u"], h["v"], h["arcs"], value, label=f"device {label}")
    print(f"device {label}: {plan['augmentations']} augmentations for n + m = {len(h['w_a']) + len(h['w_b'])}")
    assert plan["augmentations"] <= emd.DEFAULT_AUGMENTATIONS * (len(h["w_a"]) + len(h["w_b"]))


def _run(case, **kw):
    if case["kind"] == "grid":
        return emd.emd_grids(_dev(case["arr0"]), _dev(case["arr1"]), return_plan=True, **kw)
    return emd.emd_maps(_dev(case["a"]), _dev(case["b"]), _dev(case["xtf"]), _dev(case["ytf"]), return_plan=True, **kw)


@pytest.mark.parametrize("name", list(ec.cases()))
def test_value_equals_the_golden_and_the_plan_certifies_it(name):
    _lib.require_gpu()
    case = ec.cases()[name]
    want = float(ec.golden()[name + "_value"][0])
    values, plans = _run(case)
    assert values.dtype == torch.float64 and values.shape == (1,) and values.is_cuda and len(plans) == 1
    got = float(values[0])
    print(f"{name}: device {got!r}, linprog {want!r}, difference {abs(got - want):.2e}")
    assert ec.close_to_golden(got, want)
    _check_plan(plans[0], *ec.grids_of(case), got, name)
    again = _run(case)
    assert _plan_bytes(values, plans) == _plan_bytes(*again)
    if case["kind"] == "grid":                               # without the plan, a bare [H, W] pair, and the reference's norm
        bare = emd.emd_grids(_dev(case["arr0"]), _dev(case["arr1"]))
        normed = emd.emd_grids(_dev(case["arr0"]), _dev(case["arr1"]), norm=True)
        assert bare.cpu().numpy().tobytes() == values.cpu().numpy().tobytes()
        h = case["arr0"].shape[0]
        assert np.array_equal(normed.cpu().numpy(), values.cpu().numpy() / np.sqrt(h * h), equal_nan=True)


def test_conventions_of_calculate_emd():
    _lib.require_gpu()
    c = ec.cases()
    assert float(_run(c["identical"])[0][0]) == 0.0          # exactly
    assert float(_run(c["both_zero"])[0][0]) == 0.0
    assert np.isnan(float(_run(c["first_zero"])[0][0])) and np.isnan(float(_run(c["second_zero"])[0][0]))
    assert float(_run(c["single"])[0][0]) == np.sqrt(8.0)
    full = c["full_positive"]                                # the literal + abs(min) adds to a map without an empty cell
    values, plans = _run(full)
    shifted = (full["a"] + full["a"].min()) / (full["a"] + full["a"].min()).sum()
    order = np.lexsort((full["ytf"], full["xtf"]))
    assert np.abs(_host(plans[0])["w_a"] - shifted[order]).max() <= 4e-16
    unshifted = emd.emd_grids(*[_dev(np.ascontiguousarray(full[k][order].reshape(5, 4))) for k in ("a", "b")])
    assert abs(float(unshifted[0]) - float(values[0])) > 1e-3


def test_a_batch_of_different_sizes_equals_the_problems_one_by_one():
    _lib.require_gpu()
    arr0, arr1 = ec.batch_case()
    want = ec.golden()["batch_values"]
    values, plans = emd.emd_grids(_dev(arr0), _dev(arr1), return_plan=True)
    got = values.cpu().numpy()
    assert got.shape == (len(ec.BATCH_CELLS),) and len(plans) == len(got) >= 16
    for p in range(len(got)):
        assert ec.close_to_golden(got[p], want[p]), (p, got[p], want[p])
        _check_plan(plans[p], arr0[p], arr1[p], got[p], f"batch {p}")
        one, plan = emd.emd_grids(_dev(arr0[p]), _dev(arr1[p]), return_plan=True)
        assert _plan_bytes(one, plan) == _plan_bytes(values[p:p + 1], plans[p:p + 1]), p
    assert _plan_bytes(*emd.emd_grids(_dev(arr0), _dev(arr1), return_plan=True)) == _plan_bytes(values, plans)


def test_columns_of_wider_tables_and_a_gene_whose_nan_rows_shrink_its_grid():
    _lib.require_gpu()
    a, b, xtf, ytf = ec.table_case()
    want = ec.golden()["table_values"]
    values, plans = emd.emd_maps(_dev(a), _dev(b), _dev(xtf), ytf, cols_a=ec.TABLE_COLS_A, cols_b=ec.TABLE_COLS_B, return_plan=True)
    got = values.cpu().numpy()
    for p, (ja, jb) in enumerate(zip(ec.TABLE_COLS_A, ec.TABLE_COLS_B)):
        arr0, arr1 = ec.fill_shift(a[:, ja], b[:, jb], xtf, ytf)
        assert ec.close_to_golden(got[p], want[p]), (p, got[p], want[p])
        _check_plan(plans[p], arr0, arr1, got[p], f"table {p}")
    shrunk = _host(plans[ec.TABLE_NAN_PROBLEM])
    assert shrunk["coords_a"][:, 0].max() == 4 and shrunk["coords_b"][:, 1].max() == 5 and _host(plans[0])["coords_b"][:, 0].max() == 5
    normed = emd.emd_maps(_dev(a), _dev(b), _dev(xtf), _dev(ytf), cols_a=ec.TABLE_COLS_A, cols_b=ec.TABLE_COLS_B, norm=True).cpu().numpy()
    heights = np.array([ec.fill_shift(a[:, ja], b[:, jb], xtf, ytf)[0].shape[0] for ja, jb in zip(ec.TABLE_COLS_A, ec.TABLE_COLS_B)], dtype=np.float64)
    assert heights.tolist() == [6.0, 5.0, 6.0, 5.0] and np.array_equal(normed, got / np.sqrt(heights * heights))
    # no column lists: column p against column p; a vector pair; a grid that does not start at the origin of the table's rows
    plain = emd.emd_maps(_dev(a[:, :4]), _dev(b), _dev(xtf), _dev(ytf)).cpu().numpy()
    assert plain.shape == (4,) and plain[2] != got[2]
    pair = emd.emd_maps(_dev(a[:, 4].copy()), _dev(b[:, 1].copy()), _dev(xtf.astype(np.float64)), _dev(ytf.astype(np.int64)))
    assert pair.cpu().numpy().tobytes() == got[:1].tobytes()
    with pytest.raises(ValueError, match="NaN"):             # NaN rows are not dropped: refused
        emd.emd_maps(_dev(a), _dev(b), _dev(xtf), _dev(ytf), cols_a=ec.TABLE_COLS_A, cols_b=ec.TABLE_COLS_B, nan_absent=False)
    gone = b.copy()
    gone[:, 0] = np.nan                                      # a problem without any row
    assert np.isnan(emd.emd_maps(_dev(a), _dev(gone), _dev(xtf), _dev(ytf), cols_a=[0, 1], cols_b=[0, 1]).cpu().numpy()).tolist() == [True, False]


def test_a_pair_at_the_cell_limit_runs_in_the_full_lds_layout():
    """4096 cells with weight on both sides: cap_cells = SQ_EMD_MAX_CELLS, the largest LDS layout (one workgroup to a CU) and
    the last element of every per-cell array.  4096 x 4096 variables are beyond linprog here, so the value is held to the
    restatement's (tests/golden/emd.npz: limit_restated_value, admitted with its own certificate) and the proof is the
    certificate of the device's own plan."""
    import time
    _lib.require_gpu()
    arr0, arr1 = ec.limit_case()
    t0 = time.perf_counter()
    values, plans = emd.emd_grids(_dev(arr0), _dev(arr1), return_plan=True)
    got = float(values[0])
    dt = time.perf_counter() - t0
    want = float(ec.golden()["limit_restated_value"][0])
    h = _host(plans[0])
    print(f"limit: n = m = {len(h['w_a'])}, {plans[0]['augmentations']} augmentations, {plans[0]['steps']} search steps, {dt:.2f} s; "
          f"device {got!r}, restatement {want!r}, difference {abs(got - want):.2e}")
    assert len(h["w_a"]) == len(h["w_b"]) == emd.MAX_CELLS
    assert ec.close_to_golden(got, want)
    _check_plan(plans[0], arr0, arr1, got, "limit")
    assert _plan_bytes(*emd.emd_grids(_dev(arr0), _dev(arr1), return_plan=True)) == _plan_bytes(values, plans)


def test_refusals():
    _lib.require_gpu()
    ones = torch.ones(6, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="share a grid cell"):
        emd.emd_maps(ones, ones, torch.tensor([0, 1, 2, 1, 4, 5], device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="negative"):
        emd.emd_maps(ones, ones, torch.arange(6, device="cuda") - 1, torch.arange(6, device="cuda"))
    with pytest.raises(ValueError, match="column index 1"):
        emd.emd_maps(ones, ones, torch.arange(6, device="cuda"), torch.arange(6, device="cuda"), cols_a=[1], cols_b=[0])
    with pytest.raises(ValueError, match="one pair per problem"):
        emd.emd_maps(torch.ones(6, 2, dtype=torch.float64, device="cuda"), ones, torch.arange(6, device="cuda"), torch.arange(6, device="cuda"))
    g = torch.ones(3, 4, dtype=torch.float64, device="cuda")
    for bad in (-1.0, float("nan"), float("inf")):
        h = g.clone()
        h[1, 2] = bad
        with pytest.raises(ValueError, match="negative, NaN or infinite"):
            emd.emd_grids(g, h)
        with pytest.raises(ValueError, match="negative, NaN or infinite"):
            emd.emd_grids(h, g)
    big = torch.zeros(65, 64, dtype=torch.float64, device="cuda")
    big.view(-1)[: emd.MAX_CELLS + 1] = 1.0
    with pytest.raises(ValueError, match=f"{emd.MAX_CELLS + 1} cells"):          # a map above the limit, refused before any launch
        emd.emd_grids(g.new_zeros(65, 64).index_fill_(0, torch.tensor([3], device="cuda"), 0.5), big)
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        emd.emd_grids(g.cpu(), g.cpu())


def test_the_augmentation_cap_ends_a_problem_with_a_status_and_the_next_call_works():
    _lib.require_gpu()
    case = ec.cases()["raw_6x7"]
    want = float(ec.golden()["raw_6x7_value"][0])
    with pytest.raises(RuntimeError, match="problem 0.*augmentations"):
        _run(case, max_augmentations=1)
    arr0, arr1 = (np.stack([g, g]) for g in ec.grids_of(case))
    with pytest.raises(RuntimeError, match="problem 0"):
        emd.emd_grids(_dev(arr0), _dev(arr1), max_augmentations=3)
    assert ec.close_to_golden(float(_run(case)[0][0]), want)
    assert ec.close_to_golden(float(_run(case, max_augmentations=emd.DEFAULT_AUGMENTATIONS * 82)[0][0]), want)


def _whole_args():
    w = gc.whole_case()
    return (_dev(w["pred"]), gc.WHOLE_NAMES, _dev(w["xcoord"]), _dev(w["ycoord"]), w["xtf"], w["ytf"], _dev(w["spot_x"]), _dev(w["spot_y"]),
            _dev(w["spot_expr"]), gc.WHOLE_GENES)


def test_align_ground_truth_with_emd_adds_the_two_columns_in_the_reference_order():
    _lib.require_gpu()
    tiles0, genes0 = gtalign.align_ground_truth(*_whole_args(), num_tiles=4)
    tiles, genes = gtalign.align_ground_truth(*_whole_args(), num_tiles=4, emd=True)
    pd.testing.assert_frame_equal(tiles, tiles0, check_exact=True)
    assert list(genes.columns) == ["gene", "emd", "nr_gt_vals", "emd_filt", "nr_gt_vals_filt"]
    pd.testing.assert_frame_equal(genes[list(genes0.columns)], genes0, check_exact=True)
    x, y = _dev(tiles["xcoord_tf"].values), _dev(tiles["ycoord_tf"].values)
    for j, gene in enumerate(gc.WHOLE_GENES):
        raw, raw_plan = emd.emd_maps(_dev(tiles[gene].values), _dev(tiles[gene + "_ground_truth"].values), x, y, return_plan=True)
        filt, filt_plan = emd.emd_maps(_dev(tiles[gene + "_filt"].values), _dev(tiles[gene + "_ground_truth_filt"].values), x, y, return_plan=True)
        assert float(raw[0]) == genes["emd"][j] and float(filt[0]) == genes["emd_filt"][j] and np.isfinite(genes["emd"][j]) and genes["emd_filt"][j] > 0
        present = ~np.isnan(tiles[gene + "_ground_truth"].values)
        sub = tiles[present]
        for plan, col_a, col_b, value in ((raw_plan[0], gene, gene + "_ground_truth", raw), (filt_plan[0], gene + "_filt", gene + "_ground_truth_filt", filt)):
            grids = ec.fill_shift(sub[col_a].values, sub[col_b].values, sub["xcoord_tf"].values, sub["ycoord_tf"].values)
            _check_plan(plan, *grids, float(value[0]), f"{col_a} against {col_b}")
    _, genes2 = gtalign.align_ground_truth(*_whole_args(), num_tiles=4, emd=True, max_augmentations=1 << 20)
    pd.testing.assert_frame_equal(genes, genes2, check_exact=True)
    with pytest.raises(RuntimeError, match="problem 0.*augmentations"):       # the cap reaches the solver through this call
        gtalign.align_ground_truth(*_whole_args(), num_tiles=4, emd=True, max_augmentations=1)


def test_cli_emd_writes_the_five_columns_and_leaves_the_plain_files_alone(tmp_path):
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
    truth.to_csv(os.path.join(root, "truth.csv"), index=False)
    base = ["--pred_csv", os.path.join(root, "stride-1.csv"), "--ground_truth", os.path.join(root, "truth.csv"), "--gene_names", ",".join(gc.WHOLE_GENES)]
    plain, with_emd = os.path.join(root, "plain"), os.path.join(root, "with_emd")
    plain_metrics = cli.main(base + ["--out", plain])
    metrics = cli.main(base + ["--out", with_emd, "--emd", "--slide_nr", "242"])
    read = lambda folder, name: open(os.path.join(folder, name), "rb").read()              # noqa: E731
    assert sorted(os.listdir(plain)) == ["aligned.csv", "metrics.csv"] and list(plain_metrics.columns) == ["gene", "nr_gt_vals", "nr_gt_vals_filt"]
    assert read(plain, "aligned.csv") == read(with_emd, "aligned.csv")
    got = pd.read_csv(os.path.join(with_emd, "metrics.csv"), index_col=0, float_precision="round_trip")
    assert list(got.columns) == ["gene", "emd", "nr_gt_vals", "emd_filt", "nr_gt_vals_filt"]
    pd.testing.assert_frame_equal(got, metrics, check_exact=True)
    assert got.drop(columns=["emd", "emd_filt"]).to_csv().encode() == read(plain, "metrics.csv")          # byte for byte today's file
    tiles = pd.read_csv(os.path.join(with_emd, "aligned.csv"), index_col=0, float_precision="round_trip")
    x, y = _dev(tiles["xcoord_tf"].values), _dev(tiles["ycoord_tf"].values)
    for j, gene in enumerate(gc.WHOLE_GENES):
        assert float(emd.emd_maps(_dev(tiles[gene].values), _dev(tiles[gene + "_ground_truth"].values), x, y)[0]) == got["emd"][j]
        assert float(emd.emd_maps(_dev(tiles[gene + "_filt"].values), _dev(tiles[gene + "_ground_truth_filt"].values), x, y)[0]) == got["emd_filt"][j]
    first = tiles[~np.isnan(tiles[gc.WHOLE_GENES[0] + "_ground_truth"].values)]
    height = int(first["xcoord_tf"].max()) + 1
    assert read(with_emd, "slide_info.txt").decode() == f"HRI_242_T.tif \t {height * height} \t {len(first)} \n"
    with pytest.raises(RuntimeError, match="augmentations"):                                 # ... and through the command line
        cli.main(base + ["--out", os.path.join(root, "capped"), "--emd", "--max_augmentations", "2"])
    cli.main(base + ["--out", with_emd, "--emd", "--slide_nr", "242", "--max_augmentations", "100000"])       # appended, as the reference does
    assert read(with_emd, "slide_info.txt").decode().count("HRI_242_T.tif") == 2
