"""patchgen.valid_tile_grid (sq_tile_grid_valid, csrc/tilegrid.hip) against scipy's binary_dilation on every window, and
cli.visualize.valid_tiles_device / --valid_tiles device against the host's valid_tiles: valid, counts, sizes, the frames and
the written CSV equal (tests/tilegrid_cases.py holds the cases and their host results)."""
import ctypes
import os
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import tilegrid_cases as tc  # noqa: E402
from sequoia_pub_amd import _lib, patchgen  # noqa: E402
from sequoia_pub_amd.cli import visualize  # noqa: E402


def _device_mask(name):
    mask = tc.case(name)[0]
    return torch.from_numpy(mask.copy()).cuda()


def _run(name, mask=None, **kw):
    _, dims, p = tc.case(name)
    valid, counts, sizes = patchgen.valid_tile_grid(_device_mask(name) if mask is None else mask, dims, p, return_counts=True, **kw)
    assert valid.dtype == torch.bool and counts.dtype == torch.int32 and sizes.dtype == torch.int32
    assert valid.is_cuda and valid.shape == counts.shape == sizes.shape == tuple(tc.geometry(name)[2:])
    return valid.cpu().numpy(), counts.cpu().numpy(), sizes.cpu().numpy()


def _check(name, got, **kw):
    want = tc.host_grid(name, **kw)
    print(f"{name} {kw}: geometry {tc.geometry(name)}; valid {int(got[0].sum())} (host {int(want[0].sum())}); differing valid "
          f"{int((got[0] != want[0]).sum())}, counts {int((got[1] != want[1]).sum())}, sizes {int((got[2] != want[2]).sum())}")
    for g, w, what in zip(got, want, ("valid", "counts", "sizes")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, what, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_case_equals_scipy_window_by_window(name):
    _lib.require_gpu()
    _check(name, _run(name))


@pytest.mark.parametrize("name", tc.NAMES)
def test_frame_equals_valid_tiles(name):
    _lib.require_gpu()
    mask, dims, p = tc.case(name)
    got = visualize.valid_tiles_device(mask, dims, p, "cuda:0")
    pd.testing.assert_frame_equal(got, tc.host_frame(name))
    pd.testing.assert_frame_equal(visualize.valid_tiles_device(_device_mask(name), dims, p, "cuda:0"), tc.host_frame(name))


@pytest.mark.parametrize("name", ["pm8", "pm65"])
@pytest.mark.parametrize("threshold", [0.2, 0.5])
@pytest.mark.parametrize("iterations", [0, 1, 3, 8])
def test_iterations_and_threshold_against_scipy(name, iterations, threshold):
    _lib.require_gpu()
    _check(name, _run(name, iterations=iterations, threshold=threshold), iterations=iterations, threshold=threshold)


def test_mask_dtypes_and_layouts_give_the_same_result():
    _lib.require_gpu()
    for name in ("pm8", "pm33", "pm65"):
        mask, dims, p = tc.case(name)
        assert mask.dtype == np.bool_
        want = _run(name)
        as_u8 = torch.from_numpy(mask.astype(np.uint8)).cuda()
        for got in (_run(name, as_u8), _run(name, as_u8 * 255)):
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        # a transposed view of the [h, w] array: the same elements, not contiguous
        view = torch.from_numpy(np.ascontiguousarray(mask.T)).cuda().t()
        assert not view.is_contiguous() and torch.equal(view, _device_mask(name))
        assert all(np.array_equal(g, w) for g, w in zip(_run(name, view), want)), name
        # a mask of some other dtype reaches the frame through mask != 0
        pd.testing.assert_frame_equal(visualize.valid_tiles_device(mask.astype(np.float32) * 0.25, dims, p, "cuda:0"), tc.host_frame(name))
        pd.testing.assert_frame_equal(visualize.valid_tiles_device(as_u8.to(torch.int32) * 7, dims, p, "cuda:0"), tc.host_frame(name))


def test_valid_alone_equals_the_full_call():
    _lib.require_gpu()
    for name in ("pm8", "pm64", "pm65", "clipped_y"):
        _, dims, p = tc.case(name)
        alone = patchgen.valid_tile_grid(_device_mask(name), dims, p)
        assert torch.is_tensor(alone) and alone.dtype == torch.bool and np.array_equal(alone.cpu().numpy(), tc.host_grid(name)[0])


def test_two_calls_give_identical_bytes():
    _lib.require_gpu()
    for name in ("pm8", "pm64", "pm85_ds3"):                      # 32-bit words, 64-bit words, the LDS route
        x = _device_mask(name)
        first = _run(name, x)
        for _ in range(3):
            for a, b in zip(first, _run(name, x)):
                assert a.tobytes() == b.tobytes(), name


def test_empty_grid_and_non_default_stream():
    _lib.require_gpu()
    _, dims, p = tc.case("no_grid")
    valid, counts, sizes = patchgen.valid_tile_grid(_device_mask("no_grid"), dims, p, return_counts=True)
    assert valid.shape == counts.shape == sizes.shape == (0, 0) and valid.is_cuda and valid.dtype == torch.bool
    assert patchgen.valid_tile_grid(_device_mask("no_grid"), (600, 256), p).shape == (2, 0)
    assert patchgen.valid_tile_grid(_device_mask("no_grid"), (256, 600), p).shape == (0, 2)
    x = _device_mask("pm65")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run("pm65", x)
    _check("pm65", got)


def test_refusals_come_from_the_library_and_launch_nothing():
    _lib.require_gpu()
    L = _lib.lib()
    mask = torch.ones(2100, 1600, dtype=torch.uint8, device="cuda")
    valid = torch.full((4, 3), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((4, 3), -5, dtype=torch.int32, device="cuda")

    def call(pm=512, iterations=3, mask_w=2100, n_col=4, p=512, ds=1, mask_ptr=None):
        return L.sq_tile_grid_valid(_lib.ptr(mask) if mask_ptr is None else mask_ptr, mask_w, 1600, n_col, 3, p, ds, pm, iterations, 0.5,
                                    _lib.ptr(valid), _lib.ptr(counts), ctypes.c_void_p(0), _lib.stream_ptr("cuda:0"))

    for kw, message in ((dict(pm=513), "pm = 513"), (dict(pm=-1), "pm = -1"), (dict(iterations=9), "iterations = 9"),
                        (dict(mask_w=32769), "1..32768"), (dict(n_col=0), "grid of 0 x 3"), (dict(ds=0), "ds = 0"),
                        (dict(p=1 << 30), "2^31"), (dict(mask_ptr=ctypes.c_void_p(0)), "null")):
        assert call(**kw) == -1 and message in L.sq_last_error().decode(), (kw, L.sq_last_error())
    torch.cuda.synchronize()
    assert bool((valid == 7).all()) and bool((counts == -5).all())            # nothing ran
    assert call() == 0                                                        # the same buffers, good arguments: sizes null
    assert bool((valid == 1).all()) and counts.cpu().tolist() == [[512 * 512] * 3] * 4
    with pytest.raises(_lib.SequoiaHipError, match="iterations = 9"):
        patchgen.valid_tile_grid(mask, (2100, 1600), 512, iterations=9)
    with pytest.raises(_lib.SequoiaHipError, match="CUDA"):
        patchgen.valid_tile_grid(mask.cpu(), (2100, 1600), 512)
    with pytest.raises(ValueError):
        patchgen.valid_tile_grid(mask.float(), (2100, 1600), 512)


def test_visualize_cli_valid_tiles_device(tmp_path):
    """cli.visualize --valid_tiles device on a small .npy slide whose mask drops some tiles: the CSV's bytes are the
    --valid_tiles host run's."""
    from oracle import resnet_oracle as ro
    from sequoia_pub_amd.resnet import resnet50
    from sequoia_pub_amd.vis import ViS
    _lib.require_gpu()
    root = str(tmp_path)
    rs = np.random.RandomState(4)
    nx, ny, G = 9, 8, 12
    arr = rs.randint(0, 256, ((ny + 1) * 256, (nx + 1) * 256, 3), dtype=np.uint8)
    os.makedirs(os.path.join(root, "TCGA", "P"))
    np.save(os.path.join(root, "TCGA", "P", "TCGA-X.npy"), arr)
    mask = np.ones(((nx + 1) * 8, (ny + 1) * 8), dtype=bool)
    mask[:, 56:] = False                                    # background from tile row 7 on
    mask[24:41, 10:30] = False                              # a hole: two tiles gone, those around it kept by the dilation or not
    mask[3, 60] = mask[70, 62] = True                       # specks in the background: far too little
    np.save(os.path.join(root, "mask.npy"), mask)
    want = visualize.valid_tiles(mask, (arr.shape[1], arr.shape[0]), 256)
    assert 0 < len(want) < nx * (ny - 1)                    # some tiles of the tissue rows are dropped too
    genes = [f"G{i}" for i in range(G)]
    rw = os.path.join(root, "resnet.pth")
    torch.save({**resnet50().state_dict(), **ro.init_resnet50_state_dict(seed=3)}, rw)
    ck = os.path.join(root, "vis_resnet", "st")
    os.makedirs(ck)
    pickle.dump({"genes": genes}, open(os.path.join(ck, "test_results.pkl"), "wb"))
    torch.manual_seed(7)
    torch.save(ViS(G, 2048, 6, 16, 64, 64, 64, device="cpu").state_dict(), os.path.join(ck, "model_best.pt"))
    common = ["--study", "st", "--project", "P", "--gene_names", "G3,G7", "--wsi_file_name", "TCGA-X.npy", "--save_folder", "t",
              "--feat_type", "resnet", "--slide_path", os.path.join(root, "TCGA", "P"), "--mask_path", os.path.join(root, "mask.npy"),
              "--extractor_weights", rw, "--compute_dtype", "fp32", "--model_type", "vis", "--folds", "0", "--checkpoint", ck]
    res_host, path_host = visualize.main(common + ["--out_root", os.path.join(root, "out_host"), "--valid_tiles", "host"])
    res_dev, path_dev = visualize.main(common + ["--out_root", os.path.join(root, "out_device"), "--valid_tiles", "device"])
    assert os.path.basename(path_dev) == "stride-1.csv" and path_dev != path_host
    assert len(res_dev) == len(res_host) == len(want)
    pd.testing.assert_frame_equal(res_dev[list(want.columns)], want)
    assert open(path_dev, "rb").read() == open(path_host, "rb").read()
