"""Worker of tests/test_gpu_resnet_rect.py::test_bf16_halo_staged_3x3_at_256x265: the bf16 embedder on 6 tiles of 256 x 265 in a
fresh process (SQ_CONV_HALO / SQ_CONV_HALO_MIN_TILES are read once per process); saves the features to argv[1]."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import synth  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

torch.manual_seed(5)
rn = resnet50(pretrained=False, compute_dtype="bf16").to("cuda:0").eval()
for m in rn.modules():
    if isinstance(m, torch.nn.BatchNorm2d):
        m.running_mean.normal_(0, 0.1)
        m.running_var.uniform_(0.5, 1.5)
p = torch.from_numpy(np.ascontiguousarray(synth.patches_u8(3, 6, 288)[:, :256, :265])).cuda()
f = rn.extract_patches_u8(p)
torch.cuda.synchronize()
torch.save(f.cpu(), sys.argv[1])
print("features", f.shape, float(f.abs().mean()), bool(torch.isfinite(f).all()))
