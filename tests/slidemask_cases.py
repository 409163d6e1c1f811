"""Cases of the device slide mask (patchgen.slide_mask, csrc/slidemask.hip) and their host results, shared by
tests/test_slidemask_host.py and tests/test_gpu_slidemask.py.  The host result of a case is what patchgen.get_mask_image
and scipy's binary_dilation / binary_erosion compute for it; it is made once per process and never written to.

The shapes are the smallest at which a form that spans many workgroups can go wrong: single rows and columns, an image
smaller than the erosion's frame, rows of odd byte length, one extent below the closing tile (patchgen.SLIDE_MASK_TILE)
with the other across several tiles, and one slide-like image of more than two tiles in either direction whose features
(blobs on all four borders, gaps of width 1..8 and a diagonal across the tile seams, single pixels) are what a wrong halo
or a wrong border would change."""
import functools

import numpy as np
from scipy.ndimage import binary_dilation, binary_erosion

import patchfilter_cases as pc
from sequoia_pub_amd import patchgen

RGB_MIN, ITERATIONS = 50, 3
TILE_ROWS, TILE_COLS = patchgen.SLIDE_MASK_TILE
SLIDE_H, SLIDE_W = 2 * TILE_ROWS + 29, 2 * TILE_COLS + 89          # 157 x 601 for a 64 x 256 tile
BLOCK = (20, SLIDE_H - 17, 30, SLIDE_W - 171)                      # rows 20..139, columns 30..429 of tissue: the gaps cut it
GAP_WIDTHS = list(range(1, 9))
# first column of the vertical gap of width g / first row of the horizontal one; the gaps of width 4 lie across the first
# tile seams (column TILE_COLS, row TILE_ROWS), the horizontal one of width 7 across the second row seam
V_GAP_AT = {1: 100, 2: 140, 3: 180, 4: TILE_COLS - 2, 5: 300, 6: 340, 7: 380, 8: 405}
H_GAP_AT = {1: 28, 2: 36, 3: 46, 4: TILE_ROWS - 2, 5: 76, 6: 90, 7: 2 * TILE_ROWS - 3, 8: 105}
SINGLE_PIXELS = [(15, 15), (SLIDE_H - 8, 22), (TILE_ROWS, SLIDE_W - 20), (TILE_ROWS - 1, 2 * TILE_COLS - 1), (14, 2 * TILE_COLS)]
DIAGONAL = (18, SLIDE_W - 160, 130)                                 # first row, first column, length: down and to the right


def slide_layout():
    """bool [SLIDE_H, SLIDE_W]: where the slide-like image is tissue-coloured."""
    t = np.zeros((SLIDE_H, SLIDE_W), dtype=bool)
    r0, r1, c0, c1 = BLOCK
    t[r0:r1, c0:c1] = True
    for g in GAP_WIDTHS:
        t[r0:r1, V_GAP_AT[g]:V_GAP_AT[g] + g] = False
        t[H_GAP_AT[g]:H_GAP_AT[g] + g, c0:c1] = False
    t[0:10, TILE_COLS - 50:TILE_COLS + 40] = True                   # blobs on the four borders, each across a seam
    t[SLIDE_H - 7:SLIDE_H, 2 * TILE_COLS - 30:2 * TILE_COLS + 30] = True
    t[TILE_ROWS - 14:TILE_ROWS + 16, 0:12] = True
    t[2 * TILE_ROWS - 20:2 * TILE_ROWS + 12, SLIDE_W - 11:SLIDE_W] = True
    for y, x in SINGLE_PIXELS:
        t[y, x] = True
    y, x, n = DIAGONAL
    t[np.arange(y, y + n), np.arange(x, x + n)] = True
    return t


def _slide_like():
    return pc._tile(SLIDE_H, SLIDE_W, 21, slide_layout(), spread=8.0)


def _slide_dense():
    """The slide-like image with tissue-coloured pixels at random over about 30 % of it."""
    rs = np.random.RandomState(22)
    img = _slide_like().copy()
    on = rs.rand(SLIDE_H, SLIDE_W) < 0.3
    img[on] = np.clip(pc.TISSUE + rs.randn(int(on.sum()), 3) * 8.0, 0, 255).astype(np.uint8)
    return img


def _rows(h, w, first, count):
    m = np.zeros((h, w), dtype=bool)
    m[first:first + count] = True
    return m


CASES = [
    ("one_pixel", lambda: np.full((1, 1, 3), pc.TISSUE, dtype=np.uint8)),
    ("row_1x40", lambda: pc._tile(1, 40, 31, pc._columns(1, 40, 9, 20))),
    ("column_40x1", lambda: pc._tile(40, 1, 32, _rows(40, 1, 5, 22))),
    ("tiny_7x5", lambda: pc._tile(7, 5, 33, pc._columns(7, 5, 1, 3))),                 # smaller than the erosion's frame
    ("blank_90x300", lambda: pc._tile(90, 300, 34)),
    ("constant_70x300", lambda: np.full((70, 300, 3), pc.TISSUE, dtype=np.uint8)),
    ("grey_ramp_70x300", lambda: pc._grey_ramp(70, 300)),
    ("noise_66x259", lambda: pc._noise(66, 259, 35)),                                  # one row and three columns beyond a tile
    ("wide_37x1201", lambda: pc._tile(37, 1201, 36, pc._columns(37, 1201, 100, 700))),
    ("tall_1201x37", lambda: pc._tile(1201, 37, 37, _rows(1201, 37, 100, 700))),
    ("slide_like", _slide_like),
    ("slide_dense", _slide_dense),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def image(name):
    img = np.ascontiguousarray({c[0]: c[1] for c in CASES}[name]())
    img.setflags(write=False)
    return img


def closing(mask, iterations):
    """extract_patches' closing with `iterations` steps each way; scipy reads iterations < 1 as "until nothing changes", the
    library reads 0 as none."""
    if iterations == 0:
        return mask.copy()
    return binary_erosion(binary_dilation(mask, iterations=iterations), iterations=iterations)


@functools.lru_cache(maxsize=None)
def host(name, iterations=ITERATIONS):
    """dict: thresholds float64 [4], raw, closed (bool [h, w]), s_min, s_max -- the host path's values for the case."""
    img = image(name)
    if iterations != ITERATIONS:
        base = host(name)
        out = dict(base, closed=closing(base["raw"], iterations))
    else:
        s = patchgen.saturation(img)
        thr = [float(patchgen.threshold_otsu(img[:, :, c])) for c in range(3)] + [float(patchgen.threshold_otsu(s))]
        raw = patchgen.get_mask_image(img, RGB_MIN)
        out = dict(thresholds=np.array(thr, dtype=np.float64), raw=raw, closed=closing(raw, iterations), s_min=float(s.min()),
                   s_max=float(s.max()))
    for a in (out["thresholds"], out["raw"], out["closed"]):
        a.setflags(write=False)
    return out


def stats_row(h):
    """The eight doubles sq_slide_mask writes for the case, all exact."""
    return np.array(list(h["thresholds"]) + [h["raw"].sum(), h["closed"].sum(), h["s_min"], h["s_max"]], dtype=np.float64)


def gap_closed(closed, g, vertical):
    """Whether the closing filled the gap of width g of the slide-like image (looked at away from the other gaps)."""
    if vertical:
        cut = closed[H_GAP_AT[3] + 7:H_GAP_AT[3] + 12, V_GAP_AT[g]:V_GAP_AT[g] + g]          # rows 53..57: out of reach of the gaps at 46 and 62
    else:
        cut = closed[H_GAP_AT[g]:H_GAP_AT[g] + g, 50:90]                                      # columns left of every vertical gap
    assert cut.all() or not cut.any(), (g, vertical)
    return bool(cut.all())
