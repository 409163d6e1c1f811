"""The JPEG 2000 SVS reader on the device (sequoia_pub_amd.wsi.TiffSlide, csrc/j2kdec.hip) on the fixtures of tests/golden/j2k/:
the planes of every case from sq_j2k_decode_tiles against Pillow's (the parity rule of j2k_cases.check_parity) and against the
host build of the same core (tools/j2k_hostcheck.cpp) byte for byte, float path included; whole levels and regions through
read_regions; chunked batches; and the status path of damaged tiles, with bytes tests/test_j2k_host.py runs clean on the host."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import j2k_cases as jc  # noqa: E402
from sequoia_pub_amd import _lib, wsi  # noqa: E402

DEV = "cuda:0"
C = _lib._C


@pytest.fixture(scope="module")
def golden():
    _lib.require_gpu()
    return np.load(os.path.join(jc.GOLDEN_DIR, "j2k.npz"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(name, level) -> (job, planes uint8 [n, 3, h, w] of the host build of the core): computed once for the module."""
    work = tmp_path_factory.mktemp("j2k_host")
    run = jc.build_hostcheck(work, sanitize=False)
    jobs = {}
    for name in jc.CASES:
        with wsi.TiffSlide(jc.fixture(name)) as slide:
            for level in range(slide.level_count):
                jobs[(name, level)] = slide.tile_job(level)
                jc.write_job(work / f"{name}_L{level}.job", jobs[(name, level)])
    run(work)
    out = {}
    for (name, level), job in jobs.items():
        status, planes = jc.read_out(work / f"{name}_L{level}.out", job)
        assert (status == 0).all()
        out[(name, level)] = (job, planes)
    return out


def host_level(host, name, level):
    """The RGB level image the host planes make: tiles in row-major order, composed and cropped."""
    job, planes = host[(name, level)]
    spec = jc.CASES[name]
    ordered = planes[np.argsort(job["tiles"])]
    return jc.assemble(jc.compose(ordered, spec["compression"] == 33003), *spec["levels"][level], spec["tile"])


def crop_rgba(img, x0, y0, w, h):
    out = np.zeros((h, w, 4), dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, img.shape[1]), max(y0, 0), min(y0 + h, img.shape[0])
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0, :3] = img[ya:yb, xa:xb]
        out[ya - y0:yb - y0, xa - x0:xb - x0, 3] = 255
    return out


def decode_job(job):
    """sq_j2k_decode_tiles on a tile_job: (status int32 [n], planes uint8 [n, 3, h, w])."""
    dev = torch.device(DEV)
    L = _lib.lib()
    n, (w, h) = len(job["table"]), job["geom"][:2]
    streams = torch.from_numpy(job["scans"]).to(dev)
    table = torch.from_numpy(np.ascontiguousarray(job["table"])).to(dev)
    sets = torch.from_numpy(np.frombuffer(b"".join(job["sets"]), dtype=np.uint8).copy()).to(dev)
    planes = torch.empty(_lib.need(L.sq_jpeg_planes_bytes, n, w, h, 1, 1), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    need = _lib.need(L.sq_j2k_workspace_bytes, n, w, h, *job["caps"], len(job["scans"]))
    _lib.call("sq_j2k_decode_tiles", dev, streams, len(job["scans"]), table, n, sets, len(job["sets"]), w, h, *job["caps"], planes, status,
              workspace=need)
    return status.cpu().numpy(), planes.cpu().numpy().reshape(n, 3, h, w)


@pytest.mark.parametrize("name", list(jc.CASES))
def test_planes_equal_the_host_build_and_meet_the_parity_rule(name, golden, host):
    for level in range(len(jc.CASES[name]["levels"])):
        job, host_planes = host[(name, level)]
        status, planes = decode_job(job)
        assert (status == 0).all(), (name, level, status)
        assert np.array_equal(planes, host_planes), (name, level)                     # byte for byte, the float path too
        jc.check_parity(planes, golden[f"{name}/L{level}/tiles"][job["tiles"]], jc.CASES[name].get("exact", False), f"{name} L{level}")


@pytest.mark.parametrize("name", list(jc.CASES))
def test_whole_levels_through_read_regions(name, host):
    with wsi.TiffSlide(jc.fixture(name), device=DEV) as slide:
        for level, (w, h) in enumerate(jc.CASES[name]["levels"]):
            got = slide.read_regions([(0, 0)], level, (w, h))
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 4)
            got = got[0].cpu().numpy()
            assert (got[:, :, 3] == 255).all()
            assert np.array_equal(got[:, :, :3], host_level(host, name, level)), (name, level)


# (x, y, w, h) on the 400 x 260 level of 240 x 240 tiles
REGIONS = {"four_tiles": (200, 200, 80, 60), "one_pixel": (239, 240, 1, 1), "over_left": (-10, 30, 40, 20), "over_right": (380, 30, 40, 20),
           "over_top": (50, -8, 20, 30), "over_bottom": (50, 250, 20, 30), "outside": (-50, -50, 20, 20), "odd_width": (231, 235, 35, 9)}


@pytest.mark.parametrize("case", ["aperio05", "aperio03"])
def test_regions_straddle_tiles_and_levels_and_share_tiles(case, host):
    img0, img1 = host_level(host, case, 0), host_level(host, case, 1)
    with wsi.TiffSlide(jc.fixture(case), device=DEV) as slide:
        for name, (x, y, w, h) in REGIONS.items():
            got = slide.read_regions([(x, y)], 0, (w, h))[0].cpu().numpy()
            assert np.array_equal(got, crop_rgba(img0, x, y, w, h)), (case, name)
        got = slide.read_regions([(60, 40), (61, 41), (380, 250)], 1, (30, 20)).cpu().numpy()      # level 1 in level-0 pixels
        for i, (x, y) in enumerate([(30, 20), (30, 20), (190, 125)]):
            assert np.array_equal(got[i], crop_rgba(img1, x, y, 30, 20)), i
        corners = [(200, 200), (210, 205), (200, 200), (0, 0), (250, 10)]                          # repeated and overlapping
        got = slide.read_regions(corners, 0, (64, 64)).cpu().numpy()
        decoded = list(slide.last_batch_tiles)
        assert len(decoded) == len(set(decoded)) == 4                                              # every touched tile once
        for i, (x, y) in enumerate(corners):
            assert np.array_equal(got[i], crop_rgba(img0, x, y, 64, 64)), i
        slide.workspace_budget = 1                                                                 # one region per chunk
        again = slide.read_regions(corners, 0, (64, 64)).cpu().numpy()
        assert np.array_equal(again, got) and len(slide.last_batch_tiles) == 4 + 4 + 4 + 1 + 1


def test_two_calls_give_the_same_bytes_and_read_region_is_read_regions():
    with wsi.TiffSlide(jc.fixture("layers3"), device=DEV) as slide:
        a = slide.read_regions([(3, 5), (40, 0)], 0, (70, 47))
        b = slide.read_regions([(3, 5), (40, 0)], 0, (70, 47))
        assert torch.equal(a, b)
        image = slide.read_region((3, 5), 0, (70, 47))
        assert image.mode == "RGBA" and image.size == (70, 47)
        assert np.array_equal(np.asarray(image), a[0].cpu().numpy())


def test_damaged_tiles_raise_naming_them_and_leave_the_others(host, tmp_path):
    """Tile (1, 0) cut inside its last body and tile (0, 1) with a length past the stream in its first packet header
    (j2k_cases.damage_file; tests/test_j2k_host.py runs the same file through the host program under the sanitizers)."""
    path = str(tmp_path / "damaged.tif")
    jc.damage_file(jc.fixture("rct"), path)
    img = host_level(host, "rct", 0)
    with wsi.TiffSlide(path, device=DEV) as slide:
        with pytest.raises(wsi.TileDecodeError, match=r"level 0: 2 tile\(s\) did not decode") as e:
            slide.read_regions([(0, 0), (40, 35)], 0, (50, 40))
        assert "(1, 0): the code-block bytes of a packet run past" in str(e.value) and "(0, 1): a pass count, bit-plane count or length" in str(e.value)
        assert sorted(e.value.tiles) == [(0, 0, 1, C["SQ_J2K_BAD_LENGTH"]), (0, 1, 0, C["SQ_J2K_TRUNCATED_BODY"])]
        assert e.value.first_failed_region == 0
        got = e.value.regions.cpu().numpy()
        want = crop_rgba(img, 0, 0, 50, 40)
        assert np.array_equal(got[0][:32, :32], want[:32, :32]) and np.array_equal(got[0][32:, 32:], want[32:, 32:])   # tiles (0, 0), (1, 1)
        assert np.array_equal(got[1], crop_rgba(img, 40, 35, 50, 40))                                # lies on tile (1, 1) only
        ok = slide.read_regions([(32, 32)], 0, (18, 8))[0].cpu().numpy()                              # a batch that does not touch them
        assert np.array_equal(ok, crop_rgba(img, 32, 32, 18, 8))
