"""Regenerates tests/golden/resnet50_rect.npz by running the REFERENCE's ResNet-50 (src/resnet.py:155-170, plain PyTorch:
any height and width) on rectangular and odd-sized patches.  Run in the build container only (the reference tree does
not travel); only data is written, no reference source is copied.

    python tests/golden/make_resnet_rect_golden.py

The network is ``src.resnet.resnet50`` loaded with ``resnet_oracle.init_resnet50_state_dict(seed=99, perturb_bn=True)``,
exactly as make_golden.py gold_resnet does.  Stored:

    vis_u8       uint8 [2, 256, 265, 3]  (a) the visualisation path, literally (spatial_vis/visualize.py:212-216,62-66): two
                                         synth.patches_u8(5, 2, 256) patches through transforms.Resize((256, 265)) on the PIL
                                         tile.  torchvision is not installed here; on a PIL image that transform IS
                                         ``Image.resize((265, 256), BILINEAR)`` (size is (h, w), PIL takes (w, h)), so that
                                         call is made directly.  The resized patches are stored so that the GPU tests need
                                         no Pillow.
    vis_feat     f32 [2, 2048]           forward_extract of those after ToTensor (/255) and Normalize
    feat_HxW     f32 [1, 2048]           (b) forward_extract of the crop synth.patches_u8(seed, 1, 416)[:, :H, :W] for the
                                         shapes of SHAPES (seed = 20 + index); the inputs are regenerated from the seed
    param_checksum, pillow_version
"""
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from src.resnet import resnet50                      # noqa: E402  (reference)

from oracle import resnet_oracle                     # noqa: E402
import sequoia_pub_amd                               # noqa: E402,F401
from sequoia_pub_amd import synth                    # noqa: E402

SHAPES = ((250, 250), (225, 300), (300, 225), (193, 193), (193, 416), (416, 193), (416, 416), (288, 224))
VIS_SEED, CROP_SEED0 = 5, 20

torch.set_num_threads(8)


def to_model_input(p_u8):
    """ToTensor + Normalize of visualize.py:214-215 == compute_features_hdf5.py:119-120 for a uint8 HWC patch."""
    image = torch.from_numpy(p_u8).permute(2, 0, 1).to(torch.float32) / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    return ((image - mean) / std)[None]


def main():
    sd = resnet_oracle.init_resnet50_state_dict(seed=99, perturb_bn=True)
    model = resnet50(pretrained=False)
    full = model.state_dict()
    for k, v in sd.items():
        assert full[k].shape == v.shape, k
        full[k] = v
    model.load_state_dict(full)
    model.eval()
    out = {"pillow_version": np.array(PIL.__version__)}
    with torch.no_grad():
        p256 = synth.patches_u8(VIS_SEED, n_patches=2, size=256)
        vis = np.stack([np.asarray(Image.fromarray(p, "RGB").resize((265, 256), Image.BILINEAR)) for p in p256])
        assert vis.shape == (2, 256, 265, 3) and vis.dtype == np.uint8
        out["vis_u8"] = vis
        out["vis_feat"] = np.concatenate([model.forward_extract(to_model_input(p)).numpy() for p in vis])
        for i, (H, W) in enumerate(SHAPES):
            p = synth.patches_u8(CROP_SEED0 + i, n_patches=1, size=416)[:, :H, :W]
            f = model.forward_extract(to_model_input(np.ascontiguousarray(p[0]))).numpy()
            assert f.shape == (1, 2048), f.shape
            out[f"feat_{H}x{W}"] = f
    s = sum(float(v.double().sum()) for v in sd.values() if v.dtype.is_floating_point)
    a = sum(float(v.double().abs().sum()) for v in sd.values() if v.dtype.is_floating_point)
    out["param_checksum"] = np.array([s, a], dtype=np.float64)
    path = os.path.join(HERE, "resnet50_rect.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
