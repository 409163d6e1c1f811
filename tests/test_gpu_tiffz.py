"""The LZW and uncompressed tiled-TIFF reader on the device (sequoia_pub_amd.wsi.TiffSlide, csrc/tifflzw.hip): the planes of
``sq_lzw_decode_tiles`` in both modes -- a wave per tile, and a lane per tile running the serial core -- on every fixture of
tests/golden/tiffz/ against Pillow's libtiff, on the streams of tiffz_cases' encoder that libtiff never writes (pinned to
libtiff on the host by tests/test_tiffz_host.py), on one 1024 x 1024 noise tile and on batches with damaged tiles; whole levels
and regions through ``read_regions``; and patch generation and ``embed_slide`` on an LZW slide against the same pixels as an
ArraySlide.  The formats are lossless: every comparison is ``np.array_equal`` against the source pixels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiffz_cases as tz  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from sequoia_pub_amd import _lib, patchgen, store, wsi  # noqa: E402
from sequoia_pub_amd.cli.common import seed_everything  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

DEV = "cuda:0"
C = _lib._C
MODES = {"wave": C["SQ_LZW_MODE_WAVE"], "lane": C["SQ_LZW_MODE_LANE"]}


@pytest.fixture(scope="module")
def golden():
    _lib.require_gpu()
    return np.load(os.path.join(tz.GOLDEN_DIR, "tiffz.npz"))


def decode_job(job, mode):
    """sq_lzw_decode_tiles on a tile_job: (status int32 [n], planes uint8 [n, 3, h, w])."""
    dev = torch.device(DEV)
    L = _lib.lib()
    n, (w, h) = len(job["table"]), job["geom"][:2]
    compression = 5 if job["codec"] == "lzw" else 1
    scans = torch.from_numpy(job["scans"]).to(dev)
    table = torch.from_numpy(np.ascontiguousarray(job["table"])).to(dev)
    planes = torch.full((_lib.need(L.sq_jpeg_planes_bytes, n, w, h, 1, 1),), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    need = _lib.need(L.sq_lzw_workspace_bytes, n, w, h, compression)
    _lib.call("sq_lzw_decode_tiles", dev, scans, len(job["scans"]), table, n, w, h, compression, job["predictor"], MODES[mode], planes, status,
              workspace=need)
    return status.cpu().numpy(), planes.cpu().numpy().reshape(n, 3, h, w)


def both_modes(job):
    """(status, planes) of the wave mode, asserted equal to the lane mode's."""
    wave, lane = decode_job(job, "wave"), decode_job(job, "lane")
    assert np.array_equal(wave[0], lane[0]), (wave[0], lane[0])
    assert np.array_equal(wave[1], lane[1])
    return wave


def crop_rgba(img, x0, y0, w, h):
    out = np.zeros((h, w, 4), dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, img.shape[1]), max(y0, 0), min(y0 + h, img.shape[0])
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0, :3] = img[ya:yb, xa:xb]
        out[ya - y0:yb - y0, xa - x0:xb - x0, 3] = 255
    return out


# ---- the planes of both modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tz.CASES))
def test_planes_of_both_modes_are_pillows_bytes(name, golden):
    with wsi.TiffSlide(tz.fixture(name)) as slide:
        jobs = [slide.tile_job(level) for level in range(slide.level_count)]
    for level, job in enumerate(jobs):
        status, planes = both_modes(job)
        want = tz.tile_planes(tz.level_tiles(golden[f"{name}/L{level}"], tz.CASES[name]["tile"]))[job["tiles"]]
        assert (status == 0).all(), (name, level, status)
        assert np.array_equal(planes, want), (name, level)


@pytest.mark.parametrize("name", list(tz.VARIANTS))
def test_encoder_streams_libtiff_does_not_write(name):
    """Cleared when entry 4094, 4095 or 4096 would be made, after every code, every 100 codes, without EOI, and never cleared:
    the input, or for the never-cleared 64 x 64 noise tile -- which libtiff refuses -- the overrun status and zero planes."""
    stream, img, predictor = tz.variant(name)
    t = img.shape[0]
    status, planes = both_modes(tz.make_job([stream], t, t, predictor=predictor))
    if name == "never":
        assert status[0] == C["SQ_LZW_TABLE_FULL"] and (planes == 0).all()
    else:
        assert status[0] == 0 and np.array_equal(planes[0], tz.tile_planes(img[None])[0])


def test_one_noise_tile_at_the_tile_size_limit():
    """1024 x 1024 noise: 3 MB of chunky bytes through the workspace, about 800 Clears, every code width."""
    t = C["SQ_JPEG_MAX_TILE"]
    img = tz.content_image("rand", t, t, seed=2)
    stream = tz.lzw_encode(tz.predict(img, 2))
    status, planes = both_modes(tz.make_job([stream], t, t, predictor=2))
    assert status[0] == 0 and np.array_equal(planes[0], tz.tile_planes(img[None])[0])


def test_rectangular_tiles_and_rows_that_are_no_multiple_of_the_wave():
    """Tiles of 176 x 48 and 256 x 16: a row of 176 pixels leaves the last lane of the plane writer a partial chunk, 256 takes
    the dword path; both with the predictor, LZW and uncompressed."""
    for w, h in ((176, 48), (256, 16), (48, 176)):
        imgs = [tz.content_image(c, w, h, seed=4) for c in ("smooth", "rand", "flat")]
        for compression in (5, 1):
            streams = [tz.predict(i, 2) if compression == 1 else tz.lzw_encode(tz.predict(i, 2)) for i in imgs]
            status, planes = both_modes(tz.make_job(streams, w, h, compression, predictor=2))
            assert (status == 0).all() and np.array_equal(planes, tz.tile_planes(imgs)), (w, h, compression)


DAMAGED = {1: "cut1", 3: "cut40", 5: "cut700", 7: "bad_code", 8: "eoi_mid", 10: "no_clear"}


def test_a_batch_of_good_tiles_with_damaged_ones_among_them():
    """Twelve tiles of 32 x 32 with the damage tests/test_tiffz_host.py runs under the sanitizers on the host in six of them and
    two ranges outside the uploaded bytes: every such tile ends in its status with zero planes, the good ones are untouched."""
    good = [tz.content_image("smooth", 32, 32, seed=s) for s in range(12)]
    streams = [tz.lzw_encode(tz.predict(img, 2)) for img in good]
    expect = {}
    for slot, kind in DAMAGED.items():
        streams[slot], name = tz.damage(streams[slot], kind)
        expect[slot] = C[name]
    job = tz.make_job(streams, 32, 32, predictor=2)
    job["table"][4, 0] = len(job["scans"]) - 8                          # its length runs past the end of scans
    job["table"][6, 1] = 0
    expect[4] = expect[6] = C["SQ_LZW_BAD_RANGE"]
    status, planes = both_modes(job)
    want = tz.tile_planes(good)
    for slot in range(12):
        if slot in expect:
            assert status[slot] == expect[slot] and (planes[slot] == 0).all(), (slot, status)
        else:
            assert status[slot] == 0 and np.array_equal(planes[slot], want[slot]), (slot, status)
    assert sorted(set(expect.values())) == sorted(C[k] for k in ("SQ_LZW_BAD_RANGE", "SQ_LZW_TRUNCATED", "SQ_LZW_BAD_CODE", "SQ_LZW_NO_CLEAR",
                                                                 "SQ_LZW_EARLY_EOI"))


def test_the_entry_checks_before_launching():
    dev = torch.device(DEV)
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    table = torch.zeros(4, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(*, scans_bytes=16, w=16, h=16, compression=5, predictor=1, mode=0, workspace=None):
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev) if workspace is None else workspace
        _lib.call("sq_lzw_decode_tiles", dev, buf, scans_bytes, table, 1, w, h, compression, predictor, mode, buf, status, workspace=ws)
    for kw, match in ((dict(w=24), "multiples of 16"), (dict(compression=8), "compression = 8"), (dict(predictor=3), "predictor = 3"),
                      (dict(mode=2), "mode = 2"), (dict(scans_bytes=20), "multiple of 16")):
        with pytest.raises(_lib.SequoiaHipArgError, match=match):
            call(**kw)
    with pytest.raises(_lib.SequoiaHipError, match="workspace 64 < required"):
        call(workspace=torch.zeros(64, dtype=torch.uint8, device=dev))
    assert _lib.lib().sq_lzw_workspace_bytes(1, 16, 24, 5) == 0 and _lib.lib().sq_lzw_workspace_bytes(1, 16, 16, 8) == 0


# ---- through the reader -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tz.CASES))
def test_whole_levels_through_read_regions(name, golden):
    for mode in MODES.values():
        with wsi.TiffSlide(tz.fixture(name), device=DEV) as slide:
            slide.lzw_mode = mode
            for level, (w, h) in enumerate(tz.CASES[name]["levels"]):
                got = slide.read_regions([(0, 0)], level, (w, h))
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 4)
                got = got[0].cpu().numpy()
                assert (got[:, :, 3] == 255).all()
                assert np.array_equal(got[:, :, :3], golden[f"{name}/L{level}"]), (name, level)


# (x, y, w, h) on the 150 x 100 level of 32 x 32 tiles
REGIONS = {"four_tiles": (20, 20, 40, 40), "one_pixel": (77, 33, 1, 1), "over_left": (-10, 30, 40, 20), "over_right": (130, 30, 40, 20),
           "over_top": (50, -8, 20, 30), "over_bottom": (50, 90, 20, 30), "outside": (-50, -50, 20, 20), "odd_width": (31, 29, 35, 9),
           "past_the_corner": (140, 95, 30, 30)}


@pytest.mark.parametrize("case", ["smooth", "big"])
def test_regions_straddle_tiles_and_levels_and_share_tiles(case, golden):
    img0, img1 = golden[f"{case}/L0"], golden[f"{case}/L1"]
    with wsi.TiffSlide(tz.fixture(case), device=DEV) as slide:
        for name, (x, y, w, h) in REGIONS.items():
            got = slide.read_regions([(x, y)], 0, (w, h))[0].cpu().numpy()
            assert np.array_equal(got, crop_rgba(img0, x, y, w, h)), (case, name)
        got = slide.read_regions([(60, 40), (61, 41), (140, 90)], 1, (30, 20)).cpu().numpy()        # level 1 in level-0 pixels
        for i, (x, y) in enumerate([(30, 20), (30, 20), (70, 45)]):
            assert np.array_equal(got[i], crop_rgba(img1, x, y, 30, 20)), i
        corners = [(20, 20), (25, 22), (20, 20), (0, 0), (100, 10)]                                 # repeated and overlapping
        got = slide.read_regions(corners, 0, (40, 40)).cpu().numpy()
        decoded = list(slide.last_batch_tiles)
        assert len(decoded) == len(set(decoded))                                                    # every touched tile once
        for i, (x, y) in enumerate(corners):
            assert np.array_equal(got[i], crop_rgba(img0, x, y, 40, 40)), i
        slide.workspace_budget = 1                                                                  # one region per chunk
        again = slide.read_regions(corners, 0, (40, 40)).cpu().numpy()
        assert np.array_equal(again, got) and len(slide.last_batch_tiles) > len(decoded)
        image = slide.read_region((3, 5), 0, (70, 47))
        assert image.mode == "RGBA" and image.size == (70, 47) and np.array_equal(np.asarray(image), crop_rgba(img0, 3, 5, 70, 47))


def test_a_damaged_tile_raises_naming_it_and_leaves_the_others(tmp_path):
    img = tz.content_image("smooth", 60, 50, seed=8)
    count = [0]

    def encode(data):
        count[0] += 1
        s = tz.lzw_encode(data)
        return tz.damage(s, "eoi_mid")[0] if count[0] == 2 else s         # tile (1, 0)
    path = str(tmp_path / "damaged.tif")
    tz.write_slide(path, [img], 32, 5, 2, encode=encode)
    with wsi.TiffSlide(path, device=DEV) as slide:
        with pytest.raises(wsi.TileDecodeError, match=r"level 0: 1 tile\(s\) did not decode: tile \(1, 0\): the LZW end-of-information code") as e:
            slide.read_regions([(0, 0)], 0, (60, 50))
        assert e.value.tiles == [(0, 1, 0, C["SQ_LZW_EARLY_EOI"])] and e.value.first_failed_region == 0
        got = e.value.regions[0].cpu().numpy()
        want = crop_rgba(img, 0, 0, 60, 50)
        assert np.array_equal(got[:, :32], want[:, :32]) and np.array_equal(got[32:], want[32:])
        assert (got[:32, 32:, :3] == 0).all()
        ok = slide.read_regions([(0, 32)], 0, (60, 18))[0].cpu().numpy()                            # a batch that does not touch it
        assert np.array_equal(ok, crop_rgba(img, 0, 32, 60, 18))


# ---- the pipeline behind the reader ---------------------------------------------------------------------------------------------
def test_extract_patches_and_embed_slide_equal_the_array_slide(golden, tmp_path):
    levels = [golden[f"pipeline/L{i}"] for i in range(2)]
    m = resnet50(pretrained=False, compute_dtype="f16x3")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    m = m.to(DEV).eval()
    results = {}
    for kind in ("array", "tiff"):
        root = str(tmp_path / kind)
        slide = patchgen.ArraySlide(levels, {}) if kind == "array" else wsi.open_slide(tz.fixture("pipeline"), reader="tiff", device=DEV)
        if kind == "tiff":
            assert slide.properties["openslide.vendor"] == "generic-tiff" and slide.level_dimensions == ((1024, 768), (128, 96))
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
