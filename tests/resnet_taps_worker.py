"""Worker of tests/test_gpu_resnet_taps.py::test_halo_staged_3x3_taps: one forward through sq_dbg_resnet50_taps in a fresh
process (SQ_CONV_HALO is read once per process).  argv: mode, row id, output file; saves the taps and the features."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import resnet_tap_cases as tc

mode, row_id, out = sys.argv[1:4]
taps, feats = tc.run_taps(mode, "std", row_id)
torch.save(dict(taps=torch.cat([t.reshape(-1) for t in taps]), feats=feats), out)
print("taps", len(taps), "features", tuple(feats.shape), bool(torch.isfinite(feats).all()))
