"""The host side of the device slide mask (sq_slide_mask, csrc/slidemask.hip; patchgen.slide_mask): what the case list
promises about its host results, the argument checks the library makes before it touches a device, and the unchanged host
flow of extract_patches.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import slidemask_cases as sc
from sequoia_pub_amd import _lib, patchgen, store


def test_cases_are_what_the_list_says():
    assert len(sc.NAMES) == 12
    rows, cols = patchgen.SLIDE_MASK_TILE
    for name in ("slide_like", "slide_dense"):
        h, w = sc.image(name).shape[:2]
        assert h > 2 * rows and w > 2 * cols and h % rows and w % cols and h % 32 and w % 32 and h * w < 1_500_000, (name, h, w)
    for name, (short, long_) in (("wide_37x1201", (0, 1)), ("tall_1201x37", (1, 0))):
        shape = sc.image(name).shape
        assert shape[short] < patchgen.SLIDE_MASK_TILE[short] and shape[long_] > 2 * patchgen.SLIDE_MASK_TILE[long_]
        assert (shape[1] * 3) % 2 == 1                                   # rows of odd byte length: every alignment occurs
    for name in ("row_1x40", "column_40x1", "tiny_7x5"):                  # a mask, but nothing survives an erosion frame of 3
        h = sc.host(name)
        assert h["raw"].any() and not h["closed"].any(), name
    assert not sc.host("one_pixel")["raw"].any()
    for name in ("noise_66x259", "wide_37x1201", "tall_1201x37", "slide_like", "slide_dense"):
        h = sc.host(name)
        assert 0 < h["closed"].sum() < h["closed"].size and 0 < h["raw"].sum() < h["raw"].size, name
        assert not np.array_equal(h["raw"], h["closed"]), name
    # the blank image's mask is whatever Otsu makes of the noise; the constant image's thresholds are its values
    assert np.array_equal(sc.host("constant_70x300")["thresholds"][:3], sc.pc.TISSUE) and not sc.host("constant_70x300")["raw"].any()
    assert sc.host("constant_70x300")["s_min"] == sc.host("constant_70x300")["s_max"] == sc.host("constant_70x300")["thresholds"][3] > 0
    assert sc.host("grey_ramp_70x300")["s_max"] == 0.0 and sc.host("grey_ramp_70x300")["thresholds"][3] == 0.0
    extra = (sc.host("slide_dense")["raw"] & ~sc.host("slide_like")["raw"]).sum() / (~sc.host("slide_like")["raw"]).sum()
    assert 0.25 < extra < 0.35                                            # random tissue over about 30 % of what was paper


def test_slide_like_features():
    h = sc.host("slide_like")
    raw, closed, layout = h["raw"], h["closed"], sc.slide_layout()
    assert (raw != layout).mean() < 1e-3                                   # the mask is the layout up to stray pixels
    for border in (raw[0], raw[-1], raw[:, 0], raw[:, -1]):
        assert border.any()
    rows, cols = patchgen.SLIDE_MASK_TILE
    assert sc.V_GAP_AT[4] < cols < sc.V_GAP_AT[4] + 4 and sc.H_GAP_AT[4] < rows < sc.H_GAP_AT[4] + 4       # gaps across seams
    assert sc.H_GAP_AT[7] < 2 * rows < sc.H_GAP_AT[7] + 7
    for vertical in (True, False):
        filled = {g: sc.gap_closed(closed, g, vertical) for g in sc.GAP_WIDTHS}
        assert filled == {g: g <= 6 for g in sc.GAP_WIDTHS}, (vertical, filled)      # two radius-3 balls meet over 6 pixels, not over 7
    for y, x in sc.SINGLE_PIXELS:                                          # a single pixel and the diagonal survive unchanged
        assert raw[y, x] and closed[y, x] and closed[max(0, y - 1):y + 2, x - 1:x + 2].sum() == 1
    y, x, n = sc.DIAGONAL
    assert raw[np.arange(y, y + n), np.arange(x, x + n)].all() and x < 2 * cols < x + n and y < rows < 2 * rows < y + n


def test_closing_leaves_a_zero_frame():
    """scipy's defaults: dilation and erosion both see zeros outside the image."""
    ones = np.ones((10, 12), dtype=bool)
    closed = sc.closing(ones, 3)
    assert closed[3:-3, 3:-3].all() and closed.sum() == 4 * 6
    for name in sc.NAMES:
        c = sc.host(name)["closed"]
        frame = c.copy()
        frame[3:-3, 3:-3] = False
        assert not frame.any(), name
    assert np.array_equal(sc.closing(sc.host("slide_like")["raw"], 0), sc.host("slide_like")["raw"])


def test_host_results_commute_with_transposition():
    for name in ("tiny_7x5", "noise_66x259", "wide_37x1201", "slide_like"):
        img, h = sc.image(name), sc.host(name)
        t = np.ascontiguousarray(np.transpose(img, (1, 0, 2)))
        raw_t = patchgen.get_mask_image(t, sc.RGB_MIN)
        assert np.array_equal(raw_t, h["raw"].T), name
        assert np.array_equal(sc.closing(raw_t, sc.ITERATIONS), h["closed"].T), name


def test_workspace_bytes_bounds():
    L = _lib.lib()
    assert L.sq_slide_mask_workspace_bytes(1, 1) >= 4
    assert L.sq_slide_mask_workspace_bytes(32768, 32768) >= 32768 * 32768 // 8
    assert L.sq_slide_mask_workspace_bytes(32768, 1) > 0 and L.sq_slide_mask_workspace_bytes(1, 32768) > 0
    for args, word in [((0, 64), b"1..32768"), ((64, 0), b"1..32768"), ((64, 32769), b"1..32768"), ((32769, 64), b"1..32768"),
                       ((-1, 64), b"1..32768"), ((32768, 32768 + 1), b"1..32768"), ((32767, 32769), b"1..32768")]:
        assert L.sq_slide_mask_workspace_bytes(*args) == 0 and word in L.sq_last_error(), args
    assert patchgen.SLIDE_MASK_MAX_DIM == 32768 and patchgen.SLIDE_MASK_MAX_PIXELS == 2 ** 30
    # h w > 2^30 needs an extent beyond 32768 (32768 x 32768 is 2^30 exactly), so the extent message covers it


def test_launcher_checks_arguments_before_the_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 65536)()
    base = ctypes.addressof(buf)
    base += -base % 16
    need = L.sq_slide_mask_workspace_bytes(16, 40)
    assert 0 < need <= 16384

    def call(img=base, h=16, w=40, iterations=3, transpose=0, raw=None, closed=base + 4096, stats=base + 8192, ws=base + 16384, ws_bytes=need):
        return L.sq_slide_mask(img, h, w, 50, iterations, transpose, raw, closed, stats, ws, ws_bytes, None)

    for kw, word in [(dict(img=None), b"null"), (dict(closed=None), b"null"), (dict(iterations=9), b"iterations = 9"),
                     (dict(iterations=-1), b"iterations = -1"), (dict(stats=base + 8196), b"misaligned stats"), (dict(ws=None), b"workspace"),
                     (dict(ws=base + 16388), b"misaligned workspace"), (dict(ws_bytes=need - 1), b"bytes"), (dict(h=0), b"1..32768"),
                     (dict(w=32769), b"1..32768")]:
        assert call(**kw) != 0 and word in L.sq_last_error(), (kw, L.sq_last_error())


def test_python_argument_errors_need_no_kernel(tmp_path):
    import torch
    with pytest.raises(_lib.SequoiaHipError):                  # no GPU, or a CPU tensor beside one: no CPU fallback either way
        patchgen.slide_mask(torch.zeros(16, 16, 3, dtype=torch.uint8))
    slide = _slide()
    with pytest.raises(ValueError, match="device="):
        patchgen.extract_patches(slide, str(tmp_path / "m"), (32, 32), str(tmp_path / "p"), "S1", slide_mask="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        patchgen.extract_patches(slide, str(tmp_path / "m"), (32, 32), str(tmp_path / "p"), "S1", slide_mask="gpu")
    assert os.listdir(str(tmp_path)) == []                     # refused before any folder is made


def test_cli_refuses_the_device_mask_without_the_device_filter(tmp_path, capsys):
    from sequoia_pub_amd.cli import patch_gen_hdf5
    with pytest.raises(SystemExit) as e:
        patch_gen_hdf5.main(["--wsi_path", str(tmp_path), "--ref_file", "", "--slide_mask", "device"])
    assert e.value.code == 2 and "--slide_mask device needs --filter device" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        patch_gen_hdf5.main(["--wsi_path", str(tmp_path), "--ref_file", "", "--slide_mask", "card"])
    patch_gen_hdf5.main(["--wsi_path", str(tmp_path), "--ref_file", "", "--parallel", "0"])          # the default: an empty folder, nothing to do
    assert "Found 0 slides" in capsys.readouterr().out


def _slide(seed=0, tiles=(16, 12), ps=32):
    """tests/test_patchgen.py's slide: left half tissue-like, right half blank; level 1 is 8x smaller."""
    rs = np.random.RandomState(seed)
    W, H = tiles[0] * ps, tiles[1] * ps
    img = np.full((H, W, 3), 242, dtype=np.float64) + rs.randn(H, W, 3) * 2
    tissue = np.zeros((H, W), dtype=bool)
    tissue[:, : W // 2] = True
    img[tissue] = np.array([190, 110, 160]) + rs.randn(int(tissue.sum()), 3) * 25
    img = np.clip(img, 0, 255).astype(np.uint8)
    return patchgen.ArraySlide([img, img[::8, ::8].copy()])


def test_host_flow_is_unchanged_without_the_keyword(tmp_path):
    """extract_patches without `slide_mask`, and with slide_mask="host", writes what the reference's steps give: the closed
    host mask in mask.npy (C order, |b1, indexed [x, y]) and the first kept tiles of the seed-5 order."""
    slide = _slide()
    level1 = np.transpose(slide.levels[1], (1, 0, 2))
    want_mask = sc.closing(patchgen.get_mask_image(level1), 3)
    files = []
    for d, kw in (("a", {}), ("b", dict(slide_mask="host"))):
        n = patchgen.extract_patches(slide, str(tmp_path / d / "m"), (32, 32), str(tmp_path / d / "p"), "S1", max_patches_per_slide=5, **kw)
        assert n == 5
        with store.File(os.path.join(str(tmp_path / d), "p", "S1", "S1.hdf5"), "r") as f:
            data = {k: np.asarray(f[k][:]).tobytes() for k in f.keys()}
        files.append((open(str(tmp_path / d / "m" / "S1" / "mask.npy"), "rb").read(), data,
                      open(str(tmp_path / d / "p" / "S1" / "complete.txt")).read()))
    assert files[0] == files[1]
    mask_bytes, data, done = files[0]
    assert done == "Process complete!\nTotal n patch = 5" and len(data) == 5
    mask = np.load(str(tmp_path / "a" / "m" / "S1" / "mask.npy"))
    assert mask.dtype == np.bool_ and mask.flags.c_contiguous and mask.shape == (64, 48) and np.array_equal(mask, want_mask)
    assert b"'descr': '|b1', 'fortran_order': False, 'shape': (64, 48)" in mask_bytes[:128] and mask_bytes.endswith(want_mask.tobytes())
    for k, v in data.items():
        x, y = map(int, k.split("_"))
        assert v == slide.levels[0][y:y + 32, x:x + 32].tobytes() and mask[x // 8, y // 8]
