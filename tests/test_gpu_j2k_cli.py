"""``--reader tiff`` of the CLIs on a JPEG 2000 SVS-style file (tests/golden/j2k/pipeline.tif, compression 33005, lossless)
with no openslide module: cli.slide_features and cli.patch_gen_hdf5 against the same pixels -- Pillow's decode of the tile
streams -- served as an ArraySlide through a stand-in ``openslide`` module, as tests/test_gpu_wsi_cli.py does for JPEG.
Every dataset must be equal byte for byte."""
import os
import shutil
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import j2k_cases as jc  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from sequoia_pub_amd import _lib, patchgen, store  # noqa: E402
from sequoia_pub_amd.cli import patch_gen_hdf5, slide_features  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    _lib.require_gpu()
    root = str(tmp_path_factory.mktemp("j2k_cli"))
    golden = np.load(os.path.join(jc.GOLDEN_DIR, "j2k.npz"))
    levels = [jc.level_witness(golden, "pipeline", i) for i in range(2)]
    os.makedirs(os.path.join(root, "wsi"))
    shutil.copy(jc.fixture("pipeline"), os.path.join(root, "wsi", "S.svs"))
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name="S", patient_id="S", tcga_project="TCGA-X")]).to_csv(ref, index=False)
    m = resnet50(pretrained=False, compute_dtype="fp32")
    m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
    weights = os.path.join(root, "resnet50.pth")
    torch.save(m.state_dict(), weights)
    return dict(root=root, levels=levels, ref=ref, weights=weights)


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
    assert open(os.path.join(out["array"], "patches", "S", "complete.txt")).read() == open(os.path.join(out["tiff"], "patches", "S", "complete.txt")).read()
    assert open(os.path.join(out["array"], "masks", "S", "mask.npy"), "rb").read() == open(os.path.join(out["tiff"], "masks", "S", "mask.npy"), "rb").read()
