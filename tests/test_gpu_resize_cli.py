"""compute_features --feat_type uni on 256-px patches (what patch_gen_hdf5.py writes by default): ``--resize pil`` sends them
through imgproc.resize_u8_pil, the default leaves every byte of the feature file as before (uni.resize_u8); and
visualize.embed_tiles takes the same choice as an argument."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

from sequoia_pub_amd import _lib, imgproc, store  # noqa: E402
from sequoia_pub_amd.cli import compute_features  # noqa: E402
from sequoia_pub_amd.cli.common import seed_everything  # noqa: E402
from sequoia_pub_amd.uni import create_model, resize_u8  # noqa: E402


def test_compute_features_uni_resize_choice(tmp_path, monkeypatch):
    _lib.require_gpu()
    monkeypatch.setenv("SEQUOIA_ALLOW_RANDOM_UNI", "1")
    root = str(tmp_path)
    slide = "TCGA-AA-0000"
    d = os.path.join(root, "patches", slide)
    os.makedirs(d)
    rs = np.random.RandomState(4)
    f = store.File(os.path.join(d, slide + ".hdf5"), "w")
    for t in range(5):
        f.create_dataset(f"{t}_{t + 1}", data=rs.randint(0, 256, (256, 256, 3), dtype=np.uint8))
    f.close()
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name=slide, patient_id="P0", tcga_project="TCGA-BRCA", rna_G0=1.0)]).to_csv(ref, index=False)
    feats = {}
    for name, extra in (("default", []), ("float", ["--resize", "float"]), ("pil", ["--resize", "pil"])):
        out = os.path.join(root, "features_" + name)
        compute_features.main(["--feat_type", "uni", "--ref_file", ref, "--patch_data_path", os.path.join(root, "patches"),
                               "--feature_path", out] + extra)
        h = store.File(os.path.join(out, "TCGA-BRCA", slide, slide + ".h5"), "r")
        feats[name] = np.asarray(h["uni_features"][:])
        h.close()
    # the CLI's own model: the synthetic weights come from its seed
    seed_everything(99)
    model = create_model("vit_large_patch16_224", img_size=224, patch_size=16, init_values=1e-5, num_classes=0, dynamic_img_size=True)
    model.to("cuda:0").eval()
    with store.File(os.path.join(d, slide + ".hdf5"), "r") as fr:
        patches = torch.from_numpy(np.stack([np.asarray(fr[k][:]) for k in fr.keys()])).cuda()
    want_pil = model.extract_patches_u8(imgproc.resize_u8_pil(patches, 224, "bilinear"), sub_batch=1000).cpu().numpy()
    want_float = model.extract_patches_u8(resize_u8(patches, 224), sub_batch=1000).cpu().numpy()
    assert feats["pil"].shape == (5, 1024)
    assert np.array_equal(feats["pil"], want_pil)
    assert np.array_equal(feats["default"], want_float) and np.array_equal(feats["float"], want_float)
    with pytest.raises(SystemExit):
        compute_features.main(["--feat_type", "uni", "--ref_file", ref, "--patch_data_path", os.path.join(root, "patches"),
                               "--feature_path", os.path.join(root, "x"), "--resize", "nearest"])


class _MeanExtractor:
    """Stand-in extractor: the per-channel mean of every tile (enough to tell one resize from the other)."""

    def extract_patches_u8(self, t):
        return t.float().mean(dim=(1, 2)).repeat(1, 342)[:, :1024].contiguous()


def test_embed_tiles_takes_the_resize_choice():
    from sequoia_pub_amd.cli.visualize import embed_tiles
    from sequoia_pub_amd.patchgen import ArraySlide
    _lib.require_gpu()
    rng = np.random.default_rng(2)
    slide = ArraySlide([rng.integers(0, 256, (600, 1100, 3), dtype=np.uint8)])
    df = pd.DataFrame([(0, 0), (512, 0), (300, 44)], columns=["xcoord", "ycoord"])
    tiles = torch.from_numpy(np.stack([np.asarray(slide.read_region((x, y), 0, (512, 512)))[..., :3] for x, y in zip(df.xcoord, df.ycoord)])).cuda()
    ext = _MeanExtractor()
    got_pil = embed_tiles(slide, df, 512, 224, ext, "cuda:0", chunk=2, resize="pil")
    got_float = embed_tiles(slide, df, 512, 224, ext, "cuda:0", chunk=2, resize="float")
    assert torch.equal(got_pil, ext.extract_patches_u8(imgproc.resize_u8_pil(tiles, 224)))
    assert torch.equal(got_float, ext.extract_patches_u8(resize_u8(tiles, 224)))
    assert torch.equal(embed_tiles(slide, df, 512, 224, ext, "cuda:0", chunk=2), got_float)          # the default is the float path
    with pytest.raises(ValueError):
        embed_tiles(slide, df, 512, 224, ext, "cuda:0", resize="nearest")
