"""The split (lane-parallel) JPEG entropy decode on the device: ``sq_jpeg_decode_tiles_split`` against ``sq_jpeg_decode_tiles``
on the same uploads -- every fixture and level over the sweep of subsequence sizes, scans at any byte offset, the damaged
streams of tests/test_wsi_host.py -- and ``TiffSlide(entropy="split")`` against the Pillow-made goldens, on more tiles than the
device holds waves, and through patch generation, embed_slide and cli.slide_features against the serial reader.  Every
comparison is byte for byte.  The same lane functions run on the host under the sanitizers in tests/test_wsi_split_host.py."""
import os
import shutil
import struct

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import wsi_cases as wc  # noqa: E402
import wsi_split_cases as sc  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from test_wsi_host import damaged_jobs  # noqa: E402
from sequoia_pub_amd import _lib, patchgen, store, wsi  # noqa: E402
from sequoia_pub_amd.cli import slide_features  # noqa: E402
from sequoia_pub_amd.cli.common import seed_everything  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    _lib.require_gpu()
    return np.load(os.path.join(wc.GOLDEN_DIR, "wsi.npz"))


@pytest.fixture(scope="module")
def jobs():
    _lib.require_gpu()
    jobs = sc.all_jobs()
    sc.assert_the_fixtures_reach_the_corners(jobs)
    return jobs


def level_rgb(golden, name, level):
    return np.ascontiguousarray(golden[f"{name}/L{level}"].transpose(1, 2, 0))


def upload(job, table=None, sets=None, scans=None):
    table = job["table"] if table is None else table
    sets = job["sets"] if sets is None else sets
    scans = job["scans"] if scans is None else scans
    return (torch.from_numpy(np.ascontiguousarray(scans, dtype=np.uint8)).to(DEV), torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.frombuffer(b"".join(sets), dtype=np.uint8).copy()).to(DEV), len(table), len(sets), job["geom"])


def decode(up, sub=None):
    """(planes, status) of one upload through the serial entry (sub None) or the split entry with subsequences of `sub` bytes."""
    scans, table, sets, n, n_sets, geom = up
    L = _lib.lib()
    planes = torch.full((_lib.need(L.sq_jpeg_planes_bytes, n, *geom),), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    if sub is None:
        _lib.call("sq_jpeg_decode_tiles", DEV, scans, scans.numel(), table, n, sets, n_sets, *geom, planes, status,
                  workspace=_lib.need(L.sq_jpeg_workspace_bytes, n, n_sets, *geom))
    else:
        need = _lib.need(L.sq_jpeg_split_workspace_bytes, n, n_sets, *geom)
        scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
        _lib.call("sq_jpeg_decode_tiles_split", DEV, scans, scans.numel(), table, n, sets, n_sets, *geom, planes, status, scratch, need, sub)
    return planes, status


def test_split_entry_equals_the_serial_entry_on_every_fixture_over_the_sweep(jobs):
    for (name, level), job in jobs.items():
        up = upload(job)
        planes, status = decode(up)
        assert int(status.abs().sum()) == 0, (name, level)
        for sub in sc.SWEEP:
            got_planes, got_status = decode(up, sub)
            assert torch.equal(got_status, status), (name, level, sub, got_status.tolist())
            assert torch.equal(got_planes, planes), (name, level, sub)


@pytest.mark.parametrize("sub", [0, 16])
@pytest.mark.parametrize("name", list(wc.CASES))
def test_whole_levels_through_the_split_reader_equal_the_goldens(name, sub, golden):
    with wsi.TiffSlide(sc.fixture(name), device=DEV, entropy="split", sub_bytes=sub) as slide:
        for level, (w, h) in enumerate(wc.CASES[name]["levels"]):
            got = slide.read_regions([(0, 0)], level, (w, h))[0].cpu().numpy()
            assert (got[:, :, 3] == 255).all()
            assert np.array_equal(got[:, :, :3], level_rgb(golden, name, level)), (name, level)


def test_scans_at_any_byte(jobs):
    job = jobs[("noise100", 0)]
    planes, status = decode(upload(job))
    assert int(status.abs().sum()) == 0
    for shift in (1, 2, 3, 15):
        table, scans = sc.repack(job, shift)
        assert (table[:, 0] % 16 == shift).all()
        up = upload(job, table=table, scans=scans)
        ref_planes, ref_status = decode(up)
        assert torch.equal(ref_planes, planes) and torch.equal(ref_status, status)
        for sub in (16, 20, 64):
            got_planes, got_status = decode(up, sub)
            assert torch.equal(got_status, status) and torch.equal(got_planes, planes), (shift, sub)


def test_damaged_tiles_equal_the_serial_entry(jobs):
    """Streams the decoder must refuse with a status (the serial entry does, and the host program runs them under the
    sanitizers): the tile falls back to the serial scan on lane 0, so status and partial planes are the serial entry's."""
    for name, (job, table, sets, scans, expect) in damaged_jobs().items():
        up = upload(job, table, sets, scans)
        planes, status = decode(up)
        for slot, want in expect.items():
            assert int(status[slot]) == want, (name, slot)
        for sub in (16, 64):
            got_planes, got_status = decode(up, sub)
            assert torch.equal(got_status, status), (name, sub, got_status.tolist())
            assert torch.equal(got_planes, planes), (name, sub)


def crop_rgba(img, x0, y0, w, h):
    out = np.zeros((h, w, 4), dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, img.shape[1]), max(y0, 0), min(y0 + h, img.shape[0])
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0, :3] = img[ya:yb, xa:xb]
        out[ya - y0:yb - y0, xa - x0:xb - x0, 3] = 255
    return out


def test_a_truncated_tile_raises_the_same_error_and_leaves_the_same_pixels(golden, tmp_path):
    """The file of test_a_truncated_tile_raises_naming_it_and_leaves_the_others (tests/test_gpu_wsi.py), read both ways."""
    path = str(tmp_path / "cut.tif")
    shutil.copy(sc.fixture("ycc420"), path)
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
    seen = {}
    for entropy in ("serial", "split"):
        with wsi.TiffSlide(path, device=DEV, entropy=entropy) as slide:
            with pytest.raises(wsi.TileDecodeError, match=r"level 0.*tile \(1, 1\)") as e:
                slide.read_regions([(0, 0), (0, 40), (100, 0)], 0, (150, 100))
            seen[entropy] = (str(e.value), e.value.tiles, e.value.first_failed_region, e.value.regions.clone())
            ok = slide.read_regions([(64, 0)], 0, (86, 100))[0].cpu().numpy()
            assert np.array_equal(ok, crop_rgba(img, 64, 0, 86, 100))
    assert seen["split"][:3] == seen["serial"][:3]
    assert seen["split"][1] == [(0, 1, 1, _lib._C["SQ_JPEG_TRUNCATED"])] and seen["split"][2] == 0
    assert torch.equal(seen["split"][3], seen["serial"][3])                   # the failing tile's partial pixels included


def test_more_tiles_than_the_device_holds_waves(golden, tmp_path):
    """The 8281-tile level of test_more_tiles_than_waves_share_waves_and_mix_table_sets (tests/test_gpu_wsi.py): one wave per
    tile, so the grid is several times what the device holds, and seven table sets are met."""
    pool, want_tiles = [], []
    for name in ("ycc420", "optimize"):
        with wsi.TiffSlide(sc.fixture(name)) as slide:
            offsets, counts = slide.tile_ranges(0)
            ifds, _ = wsi.read_ifds(slide._fd, slide._size)
            if name == "ycc420":
                tables = bytes(ifds[slide._levels[0].index][347])
        raw = open(sc.fixture(name), "rb").read()
        pool += [raw[o:o + c] for o, c in zip(offsets, counts)]
        want_tiles += list(golden[f"{name}/L0/tiles"].transpose(0, 2, 3, 1))
    nx, ny = 91, 91
    assert nx * ny > 2 * _lib._C["SQ_JPEG_WAVE_PER_TILE_MAX"] and len(pool) == 26 and (nx * ny) % 26
    path = str(tmp_path / "many.tif")
    wc.write_tiff(path, [wc.level_ifd(nx * 32, ny * 32, 32, [pool[t % 26] for t in range(nx * ny)], 6, 2, tables)], bigtiff=True)
    want = np.stack([want_tiles[t % 26] for t in range(nx * ny)]).reshape(ny, nx, 32, 32, 3).transpose(0, 2, 1, 3, 4).reshape(ny * 32, nx * 32, 3)
    with wsi.TiffSlide(path, device=DEV, entropy="split") as slide:
        got = slide.read_regions([(0, 0)], 0, (nx * 32, ny * 32))[0].cpu().numpy()
        assert len(slide.last_batch_tiles) == nx * ny                       # one chunk, every tile once
        assert len(slide.tile_job(0)["sets"]) == 7
    assert (got[:, :, 3] == 255).all() and np.array_equal(got[:, :, :3], want)


def test_two_calls_give_the_same_bytes(jobs):
    up = upload(jobs[("pipeline", 0)])
    a, b = decode(up, 16), decode(up, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with wsi.TiffSlide(sc.fixture("noise100"), device=DEV, entropy="split") as slide:
        x = slide.read_regions([(3, 5), (40, 0)], 0, (50, 27))
        y = slide.read_regions([(3, 5), (40, 0)], 0, (50, 27))
        assert torch.equal(x, y)


def test_sub_bytes_outside_the_range_is_refused_naming_the_value(jobs):
    up = upload(jobs[("single16", 0)])
    for bad in (18, 12, 260, -16, _lib._C["SQ_JPEG_SPLIT_SUB_MAX"] + 4):
        with pytest.raises(_lib.SequoiaHipArgError, match=f"sub_bytes = {bad}"):
            decode(up, bad)
    planes, status = decode(up, _lib._C["SQ_JPEG_SPLIT_SUB_MAX"])
    ref = decode(up)
    assert torch.equal(planes, ref[0]) and torch.equal(status, ref[1])


# ---- the pipeline behind the reader ----------------------------------------------------------------------------------------
def test_patch_generation_and_embed_slide_equal_the_serial_reader(tmp_path):
    m = resnet50(pretrained=False, compute_dtype="f16x3")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    m = m.to(DEV).eval()
    results = {}
    for kind in ("serial", "split"):
        root = str(tmp_path / kind)
        slide = wsi.TiffSlide(sc.fixture("pipeline"), device=DEV, entropy=kind)
        n = patchgen.extract_patches(slide, os.path.join(root, "masks"), (256, 256), os.path.join(root, "patches"), "S", None, device=DEV,
                                     batch=5, slide_mask="device")
        with store.File(os.path.join(root, "patches", "S", "S.hdf5"), "r") as f:
            patches = {k: np.asarray(f[k][:]) for k in f.keys()}
        seed_everything(99)
        r = patchgen.embed_slide(slide, m, patch_size=(256, 256), max_patches_per_slide=None, max_patch_number=4000, n_clusters=2,
                                 feat_type="resnet", resize="float", device=DEV, batch=5, slide_mask="device")
        results[kind] = (n, patches, open(os.path.join(root, "masks", "S", "mask.npy"), "rb").read(), r)
    (na, pa, ma, ra), (nt, pt, mt, rt) = results["serial"], results["split"]
    assert na == nt and na >= 4 and list(pa) == list(pt) and ma == mt
    for k in pa:
        assert np.array_equal(pa[k], pt[k]), k
    assert np.array_equal(ra["coords"], rt["coords"]) and len(ra["coords"]) == na
    assert torch.equal(ra["features"], rt["features"]) and torch.equal(ra["cluster_features"], rt["cluster_features"])


def test_slide_features_cli_with_jpeg_entropy_split_leaves_the_serial_run_s_files(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "wsi"))
    shutil.copy(sc.fixture("pipeline"), os.path.join(root, "wsi", "S.svs"))
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name="S", patient_id="S", tcga_project="TCGA-X")]).to_csv(ref, index=False)
    m = resnet50(pretrained=False, compute_dtype="fp32")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    weights = os.path.join(root, "resnet50.pth")
    torch.save(m.state_dict(), weights)
    common = ["--feat_type", "resnet", "--ref_file", ref, "--wsi_path", os.path.join(root, "wsi"), "--weights", weights,
              "--batch", "5", "--num_clusters", "2", "--slide_mask", "device", "--seed", "3", "--reader", "tiff"]
    out = {}
    for kind in ("serial", "split"):
        out[kind] = os.path.join(root, f"sf_{kind}")
        slide_features.main(common + ["--feature_path", os.path.join(out[kind], "features"), "--mask_path", os.path.join(out[kind], "masks")]
                            + (["--jpeg_entropy", "split"] if kind == "split" else []))
    fa = store.File(os.path.join(out["serial"], "features", "TCGA-X", "S", "S.h5"), "r")
    ft = store.File(os.path.join(out["split"], "features", "TCGA-X", "S", "S.h5"), "r")
    assert sorted(fa.keys()) == sorted(ft.keys()) == ["cluster_features", "coords", "resnet_features"]
    for name in fa.keys():
        assert np.asarray(fa[name][:]).tobytes() == np.asarray(ft[name][:]).tobytes(), name
    assert np.asarray(ft["resnet_features"][:]).shape[0] >= 4
    fa.close(), ft.close()
    masks = [open(os.path.join(out[k], "masks", "S", "mask.npy"), "rb").read() for k in out]
    assert masks[0] == masks[1]
