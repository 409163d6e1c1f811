"""What the device valid-tile grid can be held to without a GPU: the cases of tests/tilegrid_cases.py are what they promise
to be (windows on both sides of the threshold and close to it, exact ties, clipped and empty windows, a leak that shows), the
argument checks that need no library, and the CLI flag's default."""
import numpy as np
import pytest
import torch

import tilegrid_cases as tc
from sequoia_pub_amd import _lib, patchgen
from sequoia_pub_amd.cli import visualize


@pytest.mark.parametrize("name", list(tc.RAMP))
def test_ramp_cases_are_what_the_table_says(name):
    valid, counts, sizes = tc.host_grid(name)
    ds, pm, n_col, n_row = tc.geometry(name)
    assert (ds, pm, n_col * n_row, int(valid.sum())) == tc.EXPECTED[name]
    assert valid.shape == counts.shape == sizes.shape == (n_col, n_row)
    assert int(valid.sum()) >= 3 and int((~valid).sum()) >= 3
    if name != "pm3":                                     # windows of 9 pixels: nothing between 4 and 5
        assert tc.near(name) >= 2, tc.near(name)
    assert len(tc.host_frame(name)) == int(valid.sum())


def test_case_sizes_straddle_the_routes():
    pms = sorted(tc.geometry(n)[1] for n in tc.RAMP)
    border = patchgen.TILE_GRID_PACKED_MAX_WINDOW
    assert border in pms and border + 1 in pms and {8, 16, 32, 33}.issubset(pms) and max(pms) == patchgen.TILE_GRID_MAX_WINDOW


def test_ties_clipped_and_empty_windows_are_there():
    assert tc.exact_ties("pm8") >= 1 and tc.exact_ties("clipped_y") >= 1 and tc.exact_ties("ties") == 2
    valid, counts, sizes = tc.host_grid("ties")
    (a, b, c) = (tc.TIE_WINDOWS[k] for k in ("first_x", "seven_of_first_x", "first_y"))
    assert (counts[a], sizes[a], bool(valid[a])) == (32, 64, True)
    assert (counts[b], sizes[b], bool(valid[b])) == (31, 64, False)
    assert (counts[c], sizes[c], bool(valid[c])) == (32, 64, True)
    assert int(valid.sum()) == 2
    valid, counts, sizes = tc.host_grid("clipped_y")
    pm = tc.geometry("clipped_y")[1]
    assert int(((sizes > 0) & (sizes < pm * pm)).sum()) == 15 and int((sizes == 0).sum()) == 30
    assert valid[sizes == 0].all()                                # an empty window is valid: 0 >= 0
    valid, counts, sizes = tc.host_grid("pm0")
    assert tc.geometry("pm0")[:2] == (300, 0) and valid.size == 99 and valid.all() and not sizes.any()
    assert len(tc.host_frame("all_zero")) == 0 and list(tc.host_frame("all_zero").columns) == ["xcoord", "ycoord"]
    assert len(tc.host_frame("all_one")) == 99 and tc.geometry("no_grid")[2:] == (0, 0) and len(tc.host_frame("no_grid")) == 0
    assert np.array_equal(tc.host_grid("bytes")[1], tc.host_grid("pm8")[1]) and set(np.unique(tc.case("bytes")[0])) == {0, 2, 255}


def test_a_leak_would_change_the_counts():
    _, counts, _ = tc.host_grid("leak")
    leaked = tc.leaked_counts("leak")
    assert counts.any() and (leaked >= counts).all() and int((leaked != counts).sum()) >= counts.size // 2
    # on the ramp the windows of this geometry leave mask columns out (255, 511): the grid does not tile the mask
    ds, pm, n_col, _ = tc.geometry("leak")
    p = tc.case("leak")[2]
    assert any((i + 1) * p // ds != i * p // ds + pm for i in range(n_col - 1))


def test_bad_geometry_is_refused_without_a_gpu():
    mask = torch.zeros(96, 80, dtype=torch.uint8)
    with pytest.raises(ValueError, match="below 1"):              # a mask wider than the slide: the host divides by zero
        patchgen.valid_tile_grid(mask, (64, 2560), 256)
    with pytest.raises(ValueError, match="below 1"):
        visualize.valid_tiles_device(mask.numpy(), (64, 2560), 256, "cuda:0")
    with pytest.raises(ValueError, match="at most 512"):          # ds 1, window 513
        patchgen.valid_tile_grid(mask, (96, 80), 513)
    with pytest.raises(ValueError, match="at most 512"):
        visualize.valid_tiles_device(mask.numpy(), (96, 80), 513, "cuda:0")
    with pytest.raises(ValueError):
        patchgen.valid_tile_grid(mask[0], (3072, 2560), 256)
    with pytest.raises(ValueError):
        patchgen.valid_tile_grid(mask, (3072, 2560), 0)
    assert patchgen.tile_grid_geometry((96, 80), (3072, 2560), 256) == (32, 8, 11, 9)
    assert patchgen.tile_grid_geometry((2100, 1600), (2100, 1600), 512) == (1, 512, 4, 3)


def test_cpu_tensor_raises_not_falls_back():
    with pytest.raises(_lib.SequoiaHipError):
        patchgen.valid_tile_grid(torch.zeros(96, 80, dtype=torch.uint8), (3072, 2560), 256)


def test_cli_flag_defaults_to_host():
    parser = visualize.build_parser()
    assert parser.parse_args([]).valid_tiles == "host"
    assert parser.parse_args(["--valid_tiles", "device"]).valid_tiles == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["--valid_tiles", "gpu"])
