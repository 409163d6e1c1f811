"""Slide regions -> cluster features without a patch store (patchgen.embed_slide, cli.slide_features) against the chain it
replaces: extract_patches(device=...) into a patch file, the body of cli.compute_features on that file, the body of
cli.kmean_features on the feature file.  The slides return RGBA from read_region, as OpenSlide does.  Every dataset must be
byte-equal, ``coords`` must be the chain's key list, ``mask.npy`` the chain's bytes, and no patch file may appear."""
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchfilter_cases as pc  # noqa: E402
from oracle import resnet_oracle  # noqa: E402  (seeded weights only)
from sequoia_pub_amd import _lib, features, patchgen, store  # noqa: E402
from sequoia_pub_amd.cli import compute_features, kmean_features, patch_gen_hdf5, slide_features  # noqa: E402
from sequoia_pub_amd.cli.common import seed_everything  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

DEV = "cuda:0"


class RGBASlide:
    """OpenSlide's interface subset over in-memory RGB levels, in the manner of patchgen.ArraySlide, but read_region returns
    RGBA [h, w, 4] as OpenSlide's does: alpha 255 inside the slide and 0 outside it, where the colour is white.  ``fail_at``:
    the level-0 read with this number (from 0) raises."""

    def __init__(self, levels, properties=None, fail_at=None):
        self.inner = patchgen.ArraySlide(levels, properties)
        self.level_dimensions, self.dimensions, self.properties = self.inner.level_dimensions, self.inner.dimensions, self.inner.properties
        self.fail_at, self.reads = fail_at, 0

    def read_region(self, location, level, size):
        if level == 0:
            self.reads += 1
            if self.fail_at is not None and self.reads - 1 == self.fail_at:
                raise OSError(f"cannot read region {location}")
        rgb = self.inner.read_region(location, level, size)
        out = np.zeros(rgb.shape[:2] + (4,), dtype=np.uint8)
        out[:, :, :3] = rgb
        a = self.inner.levels[level]
        sx = self.level_dimensions[0][0] / self.level_dimensions[level][0]
        sy = self.level_dimensions[0][1] / self.level_dimensions[level][1]
        x0, y0 = int(location[0] / sx), int(location[1] / sy)
        out[:max(0, a.shape[0] - y0), :max(0, a.shape[1] - x0), 3] = 255
        return out


def _levels(h, w, tissue, seed, down):
    img = pc._tile(h, w, seed, tissue, spread=25.0)
    return [img, np.ascontiguousarray(img[::down, ::down])]


def slide_20x(fail_at=None, seed=71):
    """6 x 5 tiles of 256: tissue left of x = 1300 and above y = 1100 but for the tile at (512, 512); the sixth column of tiles
    holds 20 tissue columns each (on the mask, dropped by the filter), the fifth row 76 tissue rows (kept).  The closing's
    erosion clears the mask's frame, so the tiles at x = 0 and y = 0 are no candidates: 15 tiles are kept."""
    h, w = 1280, 1536
    t = np.zeros((h, w), dtype=bool)
    t[:1100, :1300] = True
    t[500:780, 500:780] = False
    return RGBASlide(_levels(h, w, t, seed, 16), fail_at=fail_at)


def slide_40x():
    """3 x 3 reads of 512 pixels, shrunk to 256: tissue everywhere but the right 400 columns of the last column of tiles."""
    h = w = 1536
    t = np.ones((h, w), dtype=bool)
    t[:, 1136:] = False
    return RGBASlide(_levels(h, w, t, 72, 16), {"aperio.AppMag": "40"})


_models = {}


def model(mode):
    if mode not in _models:
        m = resnet50(pretrained=False, compute_dtype=mode)
        m.load_state_dict({**m.state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3, perturb_bn=True)})
        _models[mode] = m.to(DEV).eval()
    return _models[mode]


def chain(slide, root, m, *, slide_mask="host", max_patch_number=4000, seed=99, n_clusters=4, cap=None, feat_type="resnet", resize="float"):
    """The three steps through their files.  Returns (keys, features, cluster features or None, mask bytes)."""
    patchgen.extract_patches(slide, os.path.join(root, "masks"), (256, 256), os.path.join(root, "patches"), "S", cap, device=DEV,
                             batch=7, slide_mask=slide_mask)
    seed_everything(seed)
    with store.File(os.path.join(root, "patches", "S", "S.hdf5"), "r") as f:
        keys = features.sample_keys(f.keys(), max_patch_number)
        patches = torch.from_numpy(np.stack([np.asarray(f[k][:]) for k in keys]))
    feats = features.patch_features(m, patches, feat_type, resize, DEV).cpu().numpy()
    os.makedirs(os.path.join(root, "features"))
    path = os.path.join(root, "features", "S.h5")
    with store.File(path, "w") as f:
        f.create_dataset(f"{feat_type}_features", data=feats)
    with store.File(path, "r+") as f:
        feats = np.asarray(f[f"{feat_type}_features"][:])
        means = None
        if feats.shape[0] >= n_clusters:
            means = features.cluster(torch.from_numpy(feats).to(DEV), n_clusters, random_state=0)["cluster_features"][0].cpu().numpy()
            f.create_dataset("cluster_features", data=means)
    return keys, feats, means, open(os.path.join(root, "masks", "S", "mask.npy"), "rb").read()


def fused(slide, root, m, *, slide_mask="host", max_patch_number=4000, seed=99, n_clusters=4, cap=None, feat_type="resnet", resize="float"):
    seed_everything(seed)
    r = patchgen.embed_slide(slide, m, patch_size=(256, 256), max_patches_per_slide=cap, max_patch_number=max_patch_number,
                             n_clusters=n_clusters, feat_type=feat_type, resize=resize, device=DEV, batch=7, slide_mask=slide_mask,
                             mask_path=os.path.join(root, "masks"), slide_id="S")
    assert sorted(os.listdir(root)) == ["masks"] and os.listdir(os.path.join(root, "masks", "S")) == ["mask.npy"]      # nothing else written
    return r, open(os.path.join(root, "masks", "S", "mask.npy"), "rb").read()


def compare(tmp_path, make_slide, mode, extractor=None, width=2048, **kw):
    _lib.require_gpu()
    a, b = str(tmp_path / "chain"), str(tmp_path / "fused")
    os.makedirs(a), os.makedirs(b)
    m = extractor if extractor is not None else model(mode)
    keys, feats, means, mask = chain(make_slide(), a, m, **kw)
    r, mask_fused = fused(make_slide(), b, m, **kw)
    assert [f"{x}_{y}" for x, y in r["coords"].tolist()] == keys and r["coords"].dtype == np.int32
    assert r["features"].cpu().numpy().tobytes() == feats.tobytes() and feats.shape == (len(keys), width)
    assert (r["cluster_features"] is None) == (means is None)
    if means is not None:
        assert r["cluster_features"].cpu().numpy().tobytes() == means.tobytes()
        assert tuple(r["labels"].shape) == (len(keys),)
    assert mask_fused == mask
    return keys


@pytest.mark.parametrize("slide_mask", ["host", "device"])
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_20x_slide_equals_the_chain(tmp_path, mode, slide_mask):
    keys = compare(tmp_path, slide_20x, mode, slide_mask=slide_mask)
    assert len(keys) == 15 and "512_512" not in keys and not any(k.startswith("1280_") for k in keys)      # the filter dropped some
    assert keys == sorted(keys) and keys != sorted(keys, key=lambda k: tuple(int(v) for v in k.split("_")))    # by the bytes


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_40x_slide_equals_the_chain(tmp_path, mode):
    keys = compare(tmp_path, slide_40x, mode, slide_mask="device")
    assert len(keys) == 4


def test_more_kept_tiles_than_max_patch_number(tmp_path):
    keys = compare(tmp_path, slide_20x, "fp32", cap=12, max_patch_number=8, seed=5)
    assert len(keys) == 8 and keys != sorted(keys)                            # random.sample's order, not the file's


def test_fewer_tiles_than_clusters_and_a_failing_read(tmp_path):
    keys = compare(tmp_path, lambda: slide_20x(fail_at=10), "fp32", n_clusters=16)
    assert 0 < len(keys) <= 10


def test_uni_with_the_pil_resize(tmp_path):
    """The UNI ViT-L/16 (seeded random weights) behind the bit-exact 256 -> 224 resize, six tiles."""
    from sequoia_pub_amd.uni import create_model
    _lib.require_gpu()
    seed_everything(99)
    m = create_model("vit_large_patch16_224", img_size=224, patch_size=16, init_values=1e-5, num_classes=0, dynamic_img_size=True)
    keys = compare(tmp_path, slide_20x, None, extractor=m.to(DEV).eval(), width=1024, feat_type="uni", resize="pil", cap=6)
    assert len(keys) == 6


def _fake_openslide(monkeypatch, slides):
    """An ``openslide`` module whose OpenSlide(path) makes the slide registered under the file's name."""
    mod = types.ModuleType("openslide")
    mod.OpenSlide = lambda path: slides[os.path.basename(path)]()
    monkeypatch.setitem(sys.modules, "openslide", mod)


def test_cli_equals_the_three_clis(tmp_path, monkeypatch):
    """Three slides through the CLIs: one whose reading fails part-way (it keeps what was read before, in both routes), one
    that is not there, one complete; --max_patch_number cuts with the same --seed."""
    _lib.require_gpu()
    root = str(tmp_path)
    slides = {"A.svs": lambda: slide_20x(fail_at=17, seed=73), "C.svs": lambda: slide_20x(seed=74)}
    _fake_openslide(monkeypatch, slides)
    wsi = os.path.join(root, "wsi")
    os.makedirs(wsi)
    for name in slides:
        open(os.path.join(wsi, name), "w").close()
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name=s, patient_id=s, tcga_project="TCGA-X") for s in ("A", "B", "C")]).to_csv(ref, index=False)
    wpath = os.path.join(root, "resnet50.pth")
    torch.save(model("fp32").state_dict(), wpath)
    common = ["--feat_type", "resnet", "--ref_file", ref, "--max_patch_number", "10", "--seed", "3", "--weights", wpath]
    a, b = os.path.join(root, "chain"), os.path.join(root, "fused")
    patch_gen_hdf5.main(["--ref_file", ref, "--wsi_path", wsi, "--patch_path", os.path.join(a, "patches"), "--mask_path",
                         os.path.join(a, "masks"), "--filter", "device", "--filter_batch", "7", "--parallel", "0"])
    compute_features.main(common + ["--patch_data_path", os.path.join(a, "patches"), "--feature_path", os.path.join(a, "features")])
    kmean_features.main(["--ref_file", ref, "--feature_path", os.path.join(a, "features"), "--num_clusters", "4", "--seed", "3"])
    slide_features.main(common + ["--wsi_path", wsi, "--feature_path", os.path.join(b, "features"), "--mask_path", os.path.join(b, "masks"),
                                  "--batch", "7", "--num_clusters", "4"])
    assert sorted(os.listdir(b)) == ["features", "masks"]
    assert not [f for _, _, files in os.walk(b) for f in files if f.endswith(".hdf5")]
    for s in ("A", "C"):
        fa = store.File(os.path.join(a, "features", "TCGA-X", s, s + ".h5"), "r")
        fb = store.File(os.path.join(b, "features", "TCGA-X", s, s + ".h5"), "r")
        assert sorted(fb.keys()) == sorted(list(fa.keys()) + ["coords"])
        for name in ("resnet_features", "cluster_features"):
            assert np.asarray(fa[name][:]).tobytes() == np.asarray(fb[name][:]).tobytes(), (s, name)
        n = np.asarray(fb["resnet_features"][:]).shape[0]
        coords = np.asarray(fb["coords"][:])
        assert coords.dtype == np.int32 and coords.shape == (n, 2) and n == (10 if s == "C" else n) and 4 <= n <= 10
        fa.close(), fb.close()
        with store.File(os.path.join(a, "patches", s, s + ".hdf5"), "r") as fp:
            assert {f"{x}_{y}" for x, y in coords.tolist()} <= set(fp.keys())
        for marker in ("complete_tile.txt",):
            assert open(os.path.join(a, "features", "TCGA-X", s, marker)).read() == open(os.path.join(b, "features", "TCGA-X", s, marker)).read()
        assert open(os.path.join(a, "masks", s, "mask.npy"), "rb").read() == open(os.path.join(b, "masks", s, "mask.npy"), "rb").read()
    assert not os.path.exists(os.path.join(b, "features", "TCGA-X", "B"))
    before = os.path.getmtime(os.path.join(b, "features", "TCGA-X", "C", "C.h5"))
    slide_features.main(common + ["--wsi_path", wsi, "--feature_path", os.path.join(b, "features"), "--batch", "7", "--num_clusters", "4"])
    assert os.path.getmtime(os.path.join(b, "features", "TCGA-X", "C", "C.h5")) == before      # done slides are left alone
