"""``--reader tiff`` of the CLIs: cli.slide_features and cli.patch_gen_hdf5 on a hand-made SVS-style file (tests/golden/wsi/
pipeline.tif) with no openslide module, against the same pixels served as an ArraySlide through a stand-in ``openslide``
module -- the route tests/test_gpu_slide_features.py pins to the three-CLI chain -- and cli.visualize.embed_tiles on a TiffSlide
against read_tiles.  Every dataset must be equal byte for byte."""
import os
import shutil
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import wsi_cases as wc  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from sequoia_pub_amd import _lib, patchgen, store, wsi  # noqa: E402
from sequoia_pub_amd.cli import patch_gen_hdf5, slide_features, visualize  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    _lib.require_gpu()
    root = str(tmp_path_factory.mktemp("wsi_cli"))
    golden = np.load(os.path.join(wc.GOLDEN_DIR, "wsi.npz"))
    levels = [np.ascontiguousarray(golden[f"pipeline/L{i}"].transpose(1, 2, 0)) for i in range(2)]
    os.makedirs(os.path.join(root, "wsi"))
    shutil.copy(os.path.join(wc.GOLDEN_DIR, "pipeline.tif"), os.path.join(root, "wsi", "S.svs"))
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name="S", patient_id="S", tcga_project="TCGA-X")]).to_csv(ref, index=False)
    m = resnet50(pretrained=False, compute_dtype="fp32")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    weights = os.path.join(root, "resnet50.pth")
    torch.save(m.state_dict(), weights)
    return dict(root=root, levels=levels, ref=ref, weights=weights, model=m.to(DEV).eval())


def array_openslide(monkeypatch, levels):
    mod = types.ModuleType("openslide")
    mod.OpenSlide = lambda path: patchgen.ArraySlide(levels, {"aperio.AppMag": "20"})
    monkeypatch.setitem(sys.modules, "openslide", mod)


def test_slide_features_reader_tiff_equals_the_array_slide_route(setup, monkeypatch):
    root = setup["root"]
    common = ["--feat_type", "resnet", "--ref_file", setup["ref"], "--wsi_path", os.path.join(root, "wsi"), "--weights", setup["weights"],
              "--batch", "5", "--num_clusters", "2", "--slide_mask", "device", "--seed", "3"]
    out = {}
    for kind in ("array", "tiff"):
        if kind == "array":
            array_openslide(monkeypatch, setup["levels"])
        else:
            monkeypatch.setitem(sys.modules, "openslide", None)               # importing it fails: openslide is absent
        out[kind] = os.path.join(root, f"sf_{kind}")
        slide_features.main(common + ["--feature_path", os.path.join(out[kind], "features"), "--mask_path", os.path.join(out[kind], "masks")]
                            + (["--reader", "tiff"] if kind == "tiff" else []))
    fa = store.File(os.path.join(out["array"], "features", "TCGA-X", "S", "S.h5"), "r")
    ft = store.File(os.path.join(out["tiff"], "features", "TCGA-X", "S", "S.h5"), "r")
    assert sorted(fa.keys()) == sorted(ft.keys()) == ["cluster_features", "coords", "resnet_features"]
    for name in fa.keys():
        assert np.asarray(fa[name][:]).tobytes() == np.asarray(ft[name][:]).tobytes(), name
    assert np.asarray(ft["resnet_features"][:]).shape[0] >= 4
    fa.close(), ft.close()
    masks = [open(os.path.join(out[k], "masks", "S", "mask.npy"), "rb").read() for k in out]
    assert masks[0] == masks[1]


def test_patch_gen_reader_tiff_equals_the_array_slide_route(setup, monkeypatch):
    root = setup["root"]
    out = {}
    for kind in ("array", "tiff"):
        if kind == "array":
            array_openslide(monkeypatch, setup["levels"])
        else:
            monkeypatch.setitem(sys.modules, "openslide", None)
        out[kind] = os.path.join(root, f"pg_{kind}")
        patch_gen_hdf5.main(["--ref_file", setup["ref"], "--wsi_path", os.path.join(root, "wsi"), "--patch_path", os.path.join(out[kind], "patches"),
                             "--mask_path", os.path.join(out[kind], "masks"), "--filter", "device", "--filter_batch", "5", "--parallel", "0"]
                            + (["--reader", "tiff"] if kind == "tiff" else []))
    with store.File(os.path.join(out["array"], "patches", "S", "S.hdf5"), "r") as fa, \
            store.File(os.path.join(out["tiff"], "patches", "S", "S.hdf5"), "r") as ft:
        assert list(fa.keys()) == list(ft.keys()) and len(list(fa.keys())) >= 4
        for k in fa.keys():
            assert np.array_equal(np.asarray(fa[k][:]), np.asarray(ft[k][:])), k
    for marker in ("complete.txt",):
        assert open(os.path.join(out["array"], "patches", "S", marker)).read() == open(os.path.join(out["tiff"], "patches", "S", marker)).read()
    assert open(os.path.join(out["array"], "masks", "S", "mask.npy"), "rb").read() == open(os.path.join(out["tiff"], "masks", "S", "mask.npy"), "rb").read()


def test_missing_openslide_points_to_reader_tiff(setup, monkeypatch):
    monkeypatch.setitem(sys.modules, "openslide", None)
    for opener in (lambda: slide_features.open_slide("x.svs"), lambda: visualize.open_slide("x.svs"),
                   lambda: patch_gen_hdf5.process(("x.svs", (256, 256), "p", "m", "x", None))):
        with pytest.raises(SystemExit, match="--reader tiff"):
            opener()


def test_embed_tiles_on_a_tiff_slide_equals_read_tiles(setup):
    df = pd.DataFrame(dict(xcoord=[0, 256, 512, 300, 900], ycoord=[0, 256, 512, 100, 700]))       # the last two: off the grid, over the edge
    m = setup["model"]
    with wsi.TiffSlide(os.path.join(setup["root"], "wsi", "S.svs"), device=DEV) as slide:
        got = visualize.embed_tiles(slide, df, 256, 256, m, DEV, chunk=2)
        tiles = visualize.read_tiles(slide, df, 256)                                               # through read_region, on the host
    want = torch.cat([m.extract_patches_u8(tiles[i:i + 2].to(DEV)) for i in range(0, 5, 2)])
    level0 = setup["levels"][0]
    assert np.array_equal(tiles[3].numpy(), level0[100:356, 300:556]) and (tiles[4].numpy()[68:, :] == 0).all()
    assert torch.equal(got, want)
