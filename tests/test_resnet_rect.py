"""Rectangular and odd-sized ResNet-50 patches, the host side (no GPU): the oracle against the reference's features
(tests/golden/resnet50_rect.npz, make_resnet_rect_golden.py), the workspace sizing of sq_resnet50_workspace_bytes_hw and
resnet.max_sub_batch at (H, W)."""
import os

import numpy as np
import pytest
import torch

from oracle import resnet_oracle as ro
from sequoia_pub_amd import _lib, synth
from sequoia_pub_amd.resnet import resnet50

SHAPES = ((250, 250), (225, 300), (300, 225), (193, 193), (193, 416), (416, 193), (416, 416), (288, 224))   # make_resnet_rect_golden.py
CROP_SEED0 = 20
DTYPES = (_lib.SQ_F32, _lib.SQ_BF16, _lib.SQ_BF16X3, _lib.SQ_F16X3)


def crop(i):
    H, W = SHAPES[i]
    return np.ascontiguousarray(synth.patches_u8(CROP_SEED0 + i, n_patches=1, size=416)[:, :H, :W])


def test_oracle_matches_reference_at_every_fixture_shape(golden_dir):
    """Same tolerance as test_oracle_resnet_metrics.py holds the oracle to on resnet50.npz (rtol = atol = 1e-4)."""
    z = np.load(os.path.join(golden_dir, "resnet50_rect.npz"))
    sd = ro.init_resnet50_state_dict(seed=99, perturb_bn=True)
    s = sum(float(v.double().sum()) for v in sd.values())
    a = sum(float(v.double().abs().sum()) for v in sd.values())
    np.testing.assert_allclose([s, a], z["param_checksum"], rtol=1e-12)
    torch.set_num_threads(8)
    assert z["vis_u8"].shape == (2, 256, 265, 3)
    f = ro.embed_patches(sd, z["vis_u8"], batch=1).numpy()
    np.testing.assert_allclose(f, z["vis_feat"], rtol=1e-4, atol=1e-4)
    for i, (H, W) in enumerate(SHAPES):
        f = ro.embed_patches(sd, crop(i), batch=1).numpy()
        assert f.shape == (1, 2048)
        np.testing.assert_allclose(f, z[f"feat_{H}x{W}"], rtol=1e-4, atol=1e-4, err_msg=f"{H}x{W}")


def test_workspace_bytes_hw():
    L = _lib.lib()
    for dt in DTYPES:
        for H, W in ((256, 265),) + SHAPES:
            for n in (1, 5):
                assert L.sq_resnet50_workspace_bytes_hw(dt, n, H, W) > 0, (dt, n, H, W)
        for S in (224, 256):
            for n in (1, 3, 500):
                assert L.sq_resnet50_workspace_bytes_hw(dt, n, S, S) == L.sq_resnet50_workspace_bytes(dt, n, S) > 0
        for H, W in ((192, 192), (192, 256), (256, 192), (417, 417), (256, 417), (417, 256), (256, 500), (448, 448)):
            assert L.sq_resnet50_workspace_bytes_hw(dt, 2, H, W) == 0, (dt, H, W)
        assert L.sq_resnet50_workspace_bytes_hw(dt, 0, 256, 265) == 0
    assert L.sq_resnet50_workspace_bytes_hw(17, 1, 256, 265) == 0
    # grows with either extent
    assert L.sq_resnet50_workspace_bytes_hw(_lib.SQ_BF16, 4, 256, 265) > L.sq_resnet50_workspace_bytes_hw(_lib.SQ_BF16, 4, 256, 256)
    assert L.sq_resnet50_workspace_bytes_hw(_lib.SQ_BF16, 4, 265, 256) > L.sq_resnet50_workspace_bytes_hw(_lib.SQ_BF16, 4, 256, 256)


def planes_per_patch(H, W, fp32):
    """Bytes of the buffers the 2 GiB descriptor limit applies to, per patch, from the issue's geometry: conv1's map is
    ceil(s/2) per axis, the pooled map ceil(s/4); the widest tensors are conv1's output (64 ch), layer 1's output (256 ch)
    and, fp32 only, the stem's im2col matrix (152 columns)."""
    oh, ow = -(-H // 2), -(-W // 2)
    ph, pw = -(-oh // 2), -(-ow // 2)
    es = 4 if fp32 else 2
    out = [oh * ow * 64 * es, ph * pw * 256 * es]
    if fp32:
        out.append(oh * ow * 152 * es)
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3", "f16x3"])
def test_max_sub_batch_keeps_every_plane_under_2gib(mode):
    m = resnet50(pretrained=False, compute_dtype=mode)
    for shape in ((256, 265), (193, 193), (193, 416), (416, 416), (250, 250), (224, 224), (256, 256)):
        n = m.max_sub_batch(shape)
        assert n >= 1
        per = max(planes_per_patch(*shape, fp32=mode == "fp32"))
        assert n * per < (1 << 31), (shape, n)
        assert (n + 1) * per >= (1 << 31), (shape, n)           # and it is the largest such group
    for S in (224, 256, 416):
        assert m.max_sub_batch(S) == m.max_sub_batch((S, S))     # an int means a square


def test_unsupported_sizes_name_the_admitted_range():
    """The text of the ValueError that _run raises for a size neither entry admits, and the rule that picks the entry."""
    from sequoia_pub_amd import resnet as rn
    msg = rn._unsupported(192, 256)
    assert "193" in msg and "416" in msg and "192 x 256" in msg
    assert rn._is_square32(224, 224) and rn._is_square32(448, 448)
    assert not rn._is_square32(250, 250) and not rn._is_square32(256, 288) and not rn._is_square32(192, 192)
