"""RGBA pixels on the device and the gathers in front of the extractor: ``sq_patch_filter_px`` / ``sq_slide_mask_px`` with
pixel_bytes = 4 against the same entries with pixel_bytes = 3 on the same RGB values (which tests/test_gpu_patchfilter.py and
tests/test_gpu_slidemask.py pin to the host), ``sq_resize_u8_gather`` against ``sq_resize_u8`` on the gathered tiles (which
tests/test_gpu_resize.py pins to Pillow), ``sq_pack_rgb_gather`` against indexing.  Everything is compared with torch.equal:
only the load differs, so no output may.  The fourth byte of every RGBA input is seeded noise -- a leaking alpha byte is the
first way this goes wrong."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchfilter_cases as pc  # noqa: E402
import resize_cases as rc  # noqa: E402
import slidemask_cases as sc  # noqa: E402
from sequoia_pub_amd import _lib, imgproc, patchgen  # noqa: E402


def rgba(rgb, seed):
    """[..., 3] uint8 -> [..., 4] with seeded noise in the fourth channel."""
    rgb = np.asarray(rgb)
    a = np.random.default_rng(seed).integers(0, 256, rgb.shape[:-1] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], axis=-1))


def _flip_37x53():
    """8 tissue columns of 53: 296 mask pixels, below the bound 0.2 * 37 * 53 = 392.2; 11 columns after the dilation, 407."""
    return pc._tile(37, 53, 41, pc._columns(37, 53, 0, 8), spread=8.0)


# tiles of one shape go through one call: n = 1 .. 5, the minimum 8 x 8, rows of 159 bytes (37 x 53: no tile but the first starts
# on a dword as RGB), 256 x 256 and the full 512 x 512 bitmap
FILTER_GROUPS = {
    "8x8_n2": lambda: [pc.image("tile_8x8"), pc._tile(8, 8, 42, pc._columns(8, 8, 2, 3))],
    "37x53_n5": lambda: [pc._noise(37, 53, 43), _flip_37x53(), np.full((37, 53, 3), pc.TISSUE, dtype=np.uint8),
                         pc._tile(37, 53, 44, pc._columns(37, 53, 10, 30)), pc._tile(37, 53, 45)],
    "64x64_n4": lambda: [pc.image("case2"), pc.image("half_tissue_64"), pc.image("strip10_64"), pc.image("blank_64")],
    "256x256_n3": lambda: [pc.image("case3"), pc.image("case4"), pc._tile(256, 256, 46, pc._columns(256, 256, 30, 120))],
    "512x512_n1": lambda: [pc.image("tissue_512")],
}


@pytest.mark.parametrize("group", list(FILTER_GROUPS))
def test_patch_filter_rgba_equals_rgb(group):
    _lib.require_gpu()
    rgb = np.stack(FILTER_GROUPS[group]())
    x3 = torch.from_numpy(rgb).cuda()
    x4 = torch.from_numpy(rgba(rgb, 7)).cuda()
    want = patchgen.filter_patches(x3, pc.RGB_MIN, pc.BACKGROUND, pc.FRACTION, return_stats=True, return_masks=True)
    got = patchgen.filter_patches(x4, pc.RGB_MIN, pc.BACKGROUND, pc.FRACTION, return_stats=True, return_masks=True)
    for name, a, b in zip(("keep", "stats", "mask", "dilated"), got, want):
        assert torch.equal(a, b), (group, name)
    assert torch.equal(patchgen.filter_patches(x4), want[0])              # without the optional outputs
    if group == "37x53_n5":
        stats, bound = want[1].cpu().numpy(), pc.BACKGROUND * 37 * 53
        assert stats[1, 4] <= bound < stats[1, 5] and bool(want[0][1])     # the decision flips inside the dilation margin
        assert stats[2, 0] == pc.TISSUE[0] and stats[2, 4] == 0            # the constant tile: its value is its threshold
        assert want[0].cpu().tolist().count(True) not in (0, 5)            # kept and dropped tiles in one call


def _big_slide():
    h, w = 513, 1030                        # one row and six columns beyond 8 x 4 closing tiles
    t = np.zeros((h, w), dtype=bool)
    t[40:300, 100:700] = True
    t[60:290, 254:259] = False              # a gap across the first column seam
    t[380:513, 900:1030] = True             # a blob in the corner
    return pc._tile(h, w, 51, t, spread=8.0)


SLIDE_IMAGES = {
    "1x1": lambda: sc.image("one_pixel"),
    "70x300": lambda: pc._tile(70, 300, 52, pc._columns(70, 300, 40, 200), spread=8.0),
    "513x1030": _big_slide,
}


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("iterations", [0, 3])
@pytest.mark.parametrize("name", list(SLIDE_IMAGES))
def test_slide_mask_rgba_equals_rgb(name, iterations, transpose):
    _lib.require_gpu()
    rgb = np.array(SLIDE_IMAGES[name]())                  # a writable copy
    x3 = torch.from_numpy(rgb).cuda()
    x4 = torch.from_numpy(rgba(rgb, 8)).cuda()
    want = patchgen.slide_mask(x3, sc.RGB_MIN, iterations, transpose, return_raw=True, return_stats=True)
    got = patchgen.slide_mask(x4, sc.RGB_MIN, iterations, transpose, return_raw=True, return_stats=True)
    again = patchgen.slide_mask(x4, sc.RGB_MIN, iterations, transpose, return_raw=True, return_stats=True)
    for what, a, b, c in zip(("closed", "raw", "stats"), got, want, again):
        assert torch.equal(a, b), (name, what)
        assert torch.equal(a, c), (name, what, "two calls")
    if name != "1x1":
        assert 0 < int(want[1].sum()) < want[1].numel()


RESIZES = [((512, 512), (256, 256), "bicubic"), ((256, 256), (224, 224), "bilinear"), ((37, 53), (20, 31), "bicubic"),
           ((37, 53), (20, 31), "bilinear")]
INDEX_CASES = {"none": None, "permutation": [2, 0, 1], "subset_repeated": [1, 1], "empty": []}
_tiles_cache = {}


def _tiles(h, w, channels):
    """uint8 [3, h, w, channels] on the device: noise, structured, noise; made once per shape."""
    key = (h, w)
    if key not in _tiles_cache:
        _tiles_cache[key] = np.stack([rc.noise(h, w, 61), rc.structured(h, w, 62), rc.noise(h, w, 63)])
    rgb = _tiles_cache[key]
    return torch.from_numpy(rgb if channels == 3 else rgba(rgb, 9)).cuda()


def _index(case, dev):
    idx = INDEX_CASES[case]
    return None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)


def _gathered_rgb(src, idx):
    rows = src if idx is None else src[idx.long()]
    return rows[..., :3].contiguous()


@pytest.mark.parametrize("case", list(INDEX_CASES))
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", RESIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_{s[1][0]}x{s[1][1]}_{s[2]}")
def test_resize_gather_equals_resize_of_the_gathered(shape, channels, case):
    _lib.require_gpu()
    (h, w), size, flt = shape
    src = _tiles(h, w, channels)
    idx = _index(case, src.device)
    got = imgproc.resize_u8_pil(src, size, flt, index=idx)
    want = imgproc.resize_u8_pil(_gathered_rgb(src, idx), size, flt)          # the existing entry: three channels, no index
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape) == ((3 if idx is None else idx.numel()),) + size + (3,)
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", list(INDEX_CASES))
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("hw", [(8, 8), (37, 53), (256, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_rgb_equals_indexing(hw, channels, case):
    _lib.require_gpu()
    src = _tiles(hw[0], hw[1], channels)
    idx = _index(case, src.device)
    got = imgproc.pack_rgb(src, index=idx)
    assert got.is_contiguous() and torch.equal(got, _gathered_rgb(src, idx))
    if channels == 3:
        odd = src.flatten()[1:1 + 2 * hw[0] * hw[1] * 3].view(2, hw[0], hw[1], 3)      # tiles that start on no dword
        assert torch.equal(imgproc.pack_rgb(odd, index=idx if case != "permutation" else None),
                           _gathered_rgb(odd, idx if case != "permutation" else None))


@pytest.mark.parametrize("channels", [3, 4])
def test_out_of_range_indices_give_zero_tiles(channels):
    _lib.require_gpu()
    src = _tiles(37, 53, channels)
    idx = torch.tensor([1, -1, 0, 3, 2, 2 ** 31 - 1, -2 ** 31, 1], dtype=torch.int32, device=src.device)      # n_src = 3
    bad = torch.tensor([False, True, False, True, False, True, True, False], device=src.device)
    want = src[idx.long().clamp(0, 2)][..., :3].contiguous()
    want[bad] = 0
    assert torch.equal(imgproc.pack_rgb(src, index=idx), want)
    for size, flt in (((20, 31), "bicubic"), ((37, 53), "bilinear")):
        ref = imgproc.resize_u8_pil(src[..., :3].contiguous(), size, flt)[idx.long().clamp(0, 2)]
        ref[bad] = 0
        assert torch.equal(imgproc.resize_u8_pil(src, size, flt, index=idx), ref)


def test_arguments_are_checked():
    _lib.require_gpu()
    x = torch.zeros(2, 16, 16, 4, dtype=torch.uint8, device="cuda")
    five = torch.zeros(2, 16, 16, 5, dtype=torch.uint8, device="cuda")
    for fn in (patchgen.filter_patches, imgproc.pack_rgb, lambda t: imgproc.resize_u8_pil(t, 8)):
        with pytest.raises(ValueError, match="3 or 4"):
            fn(five)
    with pytest.raises(ValueError, match="3 or 4"):
        patchgen.slide_mask(five[0])
    with pytest.raises(ValueError, match="int32"):
        imgproc.pack_rgb(x, index=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.SequoiaHipError, match="device"):
        imgproc.pack_rgb(x, index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.SequoiaHipError, match="8..512"):
        patchgen.filter_patches(x[:, :7])
    assert tuple(imgproc.pack_rgb(x[:0]).shape) == (0, 16, 16, 3)
    assert tuple(imgproc.resize_u8_pil(x[:0], 8).shape) == (0, 8, 8, 3)
    keep = patchgen.filter_patches(x[:0])
    assert tuple(keep.shape) == (0,) and keep.dtype == torch.bool
