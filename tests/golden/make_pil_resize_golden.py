"""Regenerates tests/golden/pil_resize.npz: the outputs of PIL.Image.resize for the cases of tests/resize_cases.py
(the reference's resizes: transforms.Resize on a PIL image, pre_processing/compute_features_hdf5.py:53-56 and
spatial_vis/visualize.py:226-230, BILINEAR; patch.resize, pre_processing/patch_gen_hdf5.py:117, BICUBIC).
Only the expected outputs are stored -- the inputs come from fixed seeds -- with the Pillow version that made them:

    <case>/structured   uint8 [3, h_out, w_out]  the structured image's output, channel planes (interleaved RGB defeats
                                                 deflate: 850 KB for the eight cases against 34 KB as planes)
    <case>/noise_rows   uint8 [h_out, 32]        SHA-256 of every output row of the noise image: resampled uniform noise
                                                 does not compress (1.2 MB for the eight cases, a committed file stops at
                                                 1 MiB), and a row is bit-equal to Pillow's exactly when its digest is
    <case>/noise        uint8 [h_out, w_out, 3]  the noise output itself, for the cases of rc.FULL_NOISE

    python tests/golden/make_pil_resize_golden.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases as rc  # noqa: E402

RESAMPLE = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def pil_resize(img, h_out, w_out, resample):
    return np.asarray(Image.fromarray(img, "RGB").resize((w_out, h_out), RESAMPLE[resample]))


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (name, _, (h_out, w_out), resample) in enumerate(rc.CASES):
        x = rc.case_inputs(i)
        noise, structured = (pil_resize(im, h_out, w_out, resample) for im in x)
        out[name + "/structured"] = np.ascontiguousarray(structured.transpose(2, 0, 1))
        out[name + "/noise_rows"] = rc.row_digests(noise)
        if name in rc.FULL_NOISE:
            out[name + "/noise"] = noise
    path = os.path.join(HERE, "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
