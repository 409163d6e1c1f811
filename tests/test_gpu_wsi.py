"""The JPEG-tiled TIFF / SVS reader on the device (sequoia_pub_amd.wsi.TiffSlide, csrc/jpegdec.hip) against the Pillow-made
goldens of tests/golden/wsi/ (tests/golden/make_wsi_golden.py): whole levels of every case, regions on and over the edges,
batches that share tiles, the status path of a damaged tile, and patch generation / embed_slide on a TiffSlide against the
same slide as an ArraySlide.  Every comparison is byte for byte.  Only the goldens are read: no JPEG support is needed here."""
import os
import shutil
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wsi_cases as wc  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from sequoia_pub_amd import _lib, patchgen, store, wsi  # noqa: E402
from sequoia_pub_amd.cli.common import seed_everything  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    _lib.require_gpu()
    return np.load(os.path.join(wc.GOLDEN_DIR, "wsi.npz"))


def fixture(name):
    return os.path.join(wc.GOLDEN_DIR, f"{name}.tif")


def level_rgb(golden, name, level):
    return np.ascontiguousarray(golden[f"{name}/L{level}"].transpose(1, 2, 0))


def crop_rgba(img, x0, y0, w, h):
    """What read_region returns for the level image `img`: the crop with alpha 255, (0, 0, 0, 0) outside the level."""
    out = np.zeros((h, w, 4), dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, img.shape[1]), max(y0, 0), min(y0 + h, img.shape[0])
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0, :3] = img[ya:yb, xa:xb]
        out[ya - y0:yb - y0, xa - x0:xb - x0, 3] = 255
    return out


@pytest.mark.parametrize("name", list(wc.CASES))
def test_whole_levels_equal_the_goldens(name, golden):
    with wsi.TiffSlide(fixture(name), device=DEV) as slide:
        for level, (w, h) in enumerate(wc.CASES[name]["levels"]):
            got = slide.read_regions([(0, 0)], level, (w, h))
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 4)
            got = got[0].cpu().numpy()
            assert (got[:, :, 3] == 255).all()
            assert np.array_equal(got[:, :, :3], level_rgb(golden, name, level)), (name, level)


# (x, y, w, h) on the 150 x 100 level of 32 x 32 tiles
REGIONS = {"four_tiles": (20, 20, 40, 40), "one_pixel": (77, 33, 1, 1), "over_left": (-10, 30, 40, 20), "over_right": (130, 30, 40, 20),
           "over_top": (50, -8, 20, 30), "over_bottom": (50, 90, 20, 30), "negative": (-5, -7, 30, 30), "outside": (-50, -50, 20, 20),
           "odd_width": (31, 63, 35, 3), "beyond_corner": (140, 95, 24, 12)}


@pytest.mark.parametrize("case", ["ycc420", "ycc422", "ycc444"])
def test_regions_at_level_0(case, golden):
    img = level_rgb(golden, case, 0)
    with wsi.TiffSlide(fixture(case), device=DEV) as slide:
        for name, (x, y, w, h) in REGIONS.items():
            got = slide.read_regions([(x, y)], 0, (w, h))[0].cpu().numpy()
            assert np.array_equal(got, crop_rgba(img, x, y, w, h)), (case, name)


def test_batch_of_regions_sharing_tiles_decodes_each_tile_once(golden):
    img = level_rgb(golden, "ycc420", 0)
    corners = [(8 + 16 * i, 8 + 16 * j) for j in range(3) for i in range(3)]
    with wsi.TiffSlide(fixture("ycc420"), device=DEV) as slide:
        got = slide.read_regions(corners, 0, (40, 40)).cpu().numpy()
        decoded = list(slide.last_batch_tiles)
        for i, (x, y) in enumerate(corners):
            assert np.array_equal(got[i], crop_rgba(img, x, y, 40, 40)), i
        want = {(tx, ty) for x, y in corners for tx in range(x // 32, (x + 39) // 32 + 1) for ty in range(y // 32, (y + 39) // 32 + 1)}
        assert len(decoded) == len(set(decoded)) and set(decoded) == want and len(want) == 9          # once per batch
        # a budget of one tile: the same bytes, chunk by chunk
        slide.workspace_budget = 1
        again = slide.read_regions(corners, 0, (40, 40)).cpu().numpy()
        assert np.array_equal(again, got) and len(slide.last_batch_tiles) == sum(4 for _ in corners)


def test_level_1_is_addressed_in_level_0_pixels(golden):
    img = level_rgb(golden, "ycc422", 1)
    with wsi.TiffSlide(fixture("ycc422"), device=DEV) as slide:
        got = slide.read_regions([(60, 40), (61, 41), (140, 90)], 1, (30, 20)).cpu().numpy()
        for i, (x, y) in enumerate([(30, 20), (30, 20), (70, 45)]):                                   # int(x / 2.0), int(y / 2.0)
            assert np.array_equal(got[i], crop_rgba(img, x, y, 30, 20)), i


def test_two_calls_give_the_same_bytes_and_read_region_is_read_regions():
    with wsi.TiffSlide(fixture("noise100"), device=DEV) as slide:
        a = slide.read_regions([(3, 5), (40, 0)], 0, (50, 27))
        b = slide.read_regions([(3, 5), (40, 0)], 0, (50, 27))
        assert torch.equal(a, b)
        image = slide.read_region((3, 5), 0, (50, 27))
        assert image.mode == "RGBA" and image.size == (50, 27)
        assert np.array_equal(np.asarray(image), a[0].cpu().numpy())


def test_a_truncated_tile_raises_naming_it_and_leaves_the_others(golden, tmp_path):
    """Tile (1, 1) of level 0 cut at a third of its scan (the host check program runs the same stream clean under the
    sanitizers: tests/test_wsi_host.py): the lane stops with a status, nothing else happens to the batch."""
    path = str(tmp_path / "cut.tif")
    shutil.copy(fixture("ycc420"), path)
    with wsi.TiffSlide(path) as slide:
        offsets, counts = slide.tile_ranges(0)
        t = 1 * 5 + 1
        info = slide._tile_info(slide._levels[0], t)
        new_count = (info[0] - int(offsets[t])) + info[1] // 3
    raw = bytearray(open(path, "rb").read())
    at = raw.index(np.asarray(counts, dtype="<u4").tobytes())
    struct.pack_into("<I", raw, at + 4 * t, new_count)
    open(path, "wb").write(raw)
    img = level_rgb(golden, "ycc420", 0)
    with wsi.TiffSlide(path, device=DEV) as slide:
        with pytest.raises(RuntimeError, match=r"level 0.*tile \(1, 1\)") as e:
            slide.read_regions([(0, 0), (0, 40), (100, 0)], 0, (150, 100))
        assert e.value.tiles == [(0, 1, 1, _lib._C["SQ_JPEG_TRUNCATED"])] and e.value.first_failed_region == 0
        got = e.value.regions.cpu().numpy()
        for i, (x, y) in enumerate([(0, 0), (0, 40), (100, 0)]):
            want = crop_rgba(img, x, y, 150, 100)
            keep = np.ones((100, 150), dtype=bool)
            keep[max(32 - y, 0):max(64 - y, 0), max(32 - x, 0):max(64 - x, 0)] = False                # the failing tile's pixels
            assert np.array_equal(got[i][keep], want[keep]), i
        ok = slide.read_regions([(64, 0)], 0, (86, 100))[0].cpu().numpy()                             # a batch that does not touch it
        assert np.array_equal(ok, crop_rgba(img, 64, 0, 86, 100))


def test_more_tiles_than_waves_share_waves_and_mix_table_sets(golden, tmp_path):
    """Above SQ_JPEG_WAVE_PER_TILE_MAX tiles the entropy kernel puts 2 to 64 tiles on one wave, and a lane whose table set is
    not the wave's first reads its tables from global memory.  A level of 91 x 91 tiles of 32 pixels made of the tiles of two
    fixtures -- ycc420's, which use the JPEGTables stream, and optimize's, each with Huffman and quantisation tables of its
    own -- read whole: 8281 tiles in one chunk, four lanes per wave, seven table sets met in the scan-length order."""
    pool, want_tiles = [], []
    for name in ("ycc420", "optimize"):
        with wsi.TiffSlide(fixture(name)) as slide:
            offsets, counts = slide.tile_ranges(0)
            ifds, _ = wsi.read_ifds(slide._fd, slide._size)
            if name == "ycc420":
                tables = bytes(ifds[slide._levels[0].index][347])
        raw = open(fixture(name), "rb").read()
        pool += [raw[o:o + c] for o, c in zip(offsets, counts)]
        want_tiles += list(golden[f"{name}/L0/tiles"].transpose(0, 2, 3, 1))
    nx, ny = 91, 91              # 8281 tiles: four lanes per wave; 318 or 319 copies of each tile, so waves straddle the table sets
    assert nx * ny > 2 * _lib._C["SQ_JPEG_WAVE_PER_TILE_MAX"] and len(pool) == 26 and (nx * ny) % 26
    path = str(tmp_path / "many.tif")
    wc.write_tiff(path, [wc.level_ifd(nx * 32, ny * 32, 32, [pool[t % 26] for t in range(nx * ny)], 6, 2, tables)], bigtiff=True)
    want = np.stack([want_tiles[t % 26] for t in range(nx * ny)]).reshape(ny, nx, 32, 32, 3).transpose(0, 2, 1, 3, 4).reshape(ny * 32, nx * 32, 3)
    with wsi.TiffSlide(path, device=DEV) as slide:
        got = slide.read_regions([(0, 0)], 0, (nx * 32, ny * 32))[0].cpu().numpy()
        assert len(slide.last_batch_tiles) == nx * ny                       # one chunk, every tile once
        assert len(slide.tile_job(0)["sets"]) == 7
    assert (got[:, :, 3] == 255).all() and np.array_equal(got[:, :, :3], want)


# ---- patch generation and embed_slide on a TiffSlide against the same pixels as an ArraySlide ------------------------------
def test_extract_patches_and_embed_slide_equal_the_array_slide(golden, tmp_path):
    levels = [level_rgb(golden, "pipeline", i) for i in range(2)]
    props = {"aperio.AppMag": "20"}
    m = resnet50(pretrained=False, compute_dtype="f16x3")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    m = m.to(DEV).eval()
    results = {}
    for kind in ("array", "tiff"):
        root = str(tmp_path / kind)
        slide = patchgen.ArraySlide(levels, props) if kind == "array" else wsi.TiffSlide(fixture("pipeline"), device=DEV)
        if kind == "tiff":
            assert slide.properties["aperio.AppMag"] == "20" and slide.level_dimensions == ((1024, 768), (128, 96))
        n = patchgen.extract_patches(slide, os.path.join(root, "masks"), (256, 256), os.path.join(root, "patches"), "S", None, device=DEV,
                                     batch=5, slide_mask="device")
        with store.File(os.path.join(root, "patches", "S", "S.hdf5"), "r") as f:
            patches = {k: np.asarray(f[k][:]) for k in f.keys()}
        seed_everything(99)
        r = patchgen.embed_slide(slide, m, patch_size=(256, 256), max_patches_per_slide=None, max_patch_number=4000, n_clusters=2,
                                 feat_type="resnet", resize="float", device=DEV, batch=5, slide_mask="device")
        results[kind] = (n, patches, open(os.path.join(root, "masks", "S", "mask.npy"), "rb").read(), r)
    (na, pa, ma, ra), (nt, pt, mt, rt) = results["array"], results["tiff"]
    assert na == nt and na >= 4 and list(pa) == list(pt) and ma == mt
    for k in pa:
        assert pa[k].shape == (256, 256, 3) and np.array_equal(pa[k], pt[k]), k
    assert np.array_equal(ra["coords"], rt["coords"]) and len(ra["coords"]) == na
    assert torch.equal(ra["features"], rt["features"]) and torch.equal(ra["cluster_features"], rt["cluster_features"])


class FailingArraySlide(patchgen.ArraySlide):
    """An ArraySlide whose level-0 read fails where it touches one 256-pixel tile: the region-by-region route's behaviour."""

    def __init__(self, levels, properties, bad_tile):
        super().__init__(levels, properties)
        self.bad_tile = bad_tile

    def read_region(self, location, level, size):
        x0, y0 = self.bad_tile[0] * 256, self.bad_tile[1] * 256
        if level == 0 and location[0] < x0 + 256 and location[0] + size[0] > x0 and location[1] < y0 + 256 and location[1] + size[1] > y0:
            raise RuntimeError("unreadable region")
        return super().read_region(location, level, size)


def test_a_failing_tile_keeps_the_read_error_rule_of_patch_generation(golden, tmp_path):
    """Tile (2, 2) of the pipeline slide truncated (the fifth region of the visiting order, three kept in front of it): extract_patches on the TiffSlide writes the tiles kept before the failing
    region and then reports the error, exactly as the region-by-region route does for a slide that fails at the same region."""
    levels = [level_rgb(golden, "pipeline", i) for i in range(2)]
    path = str(tmp_path / "cut.tif")
    shutil.copy(fixture("pipeline"), path)
    with wsi.TiffSlide(path) as slide:
        offsets, counts = slide.tile_ranges(0)
        t = 2 * 4 + 2
        info = slide._tile_info(slide._levels[0], t)
        new_count = (info[0] - int(offsets[t])) + info[1] // 3
    raw = bytearray(open(path, "rb").read())
    at = raw.index(np.asarray(counts, dtype="<u4").tobytes())
    struct.pack_into("<I", raw, at + 4 * t, new_count)
    open(path, "wb").write(raw)
    written = {}
    for kind in ("array", "tiff"):
        root = str(tmp_path / kind)
        slide = FailingArraySlide(levels, {"aperio.AppMag": "20"}, (2, 2)) if kind == "array" else wsi.TiffSlide(path, device=DEV)
        n = patchgen.extract_patches(slide, os.path.join(root, "masks"), (256, 256), os.path.join(root, "patches"), "S", None, device=DEV,
                                     batch=5, slide_mask="device")
        assert n is None and not os.path.exists(os.path.join(root, "patches", "S", "complete.txt"))      # the error was reported
        with store.File(os.path.join(root, "patches", "S", "S.hdf5"), "r") as f:
            written[kind] = {k: np.asarray(f[k][:]) for k in f.keys()}
    assert list(written["array"]) == list(written["tiff"]) and len(written["tiff"]) == 3 and "512_512" not in written["tiff"]
    for k in written["array"]:
        assert np.array_equal(written["array"][k], written["tiff"][k]), k

