"""UNI embedder in the split-fp16 mode (f16x3): every product on fp16 hi / lo planes (three fp16 MFMAs), the residual
stream in fp32.  Held to the oracle (oracle/uni_oracle.py) at the fp32 tolerance, to the exact (fp64) features at the bars
the ResNet-50 split mode meets, to the fp32 mode's k-Means labels, and to the fp32 mode's bits wherever an fp16 overflow
sends a launch group back to fp32."""
import os
import warnings

import numpy as np
import pytest
import torch

from gpu_util import rel_err

pytestmark = pytest.mark.gpu

from oracle import uni_oracle  # noqa: E402  (checker only)
from sequoia_pub_amd import _lib, store, synth  # noqa: E402
from sequoia_pub_amd.kmeans import kmeans_fit_batch  # noqa: E402
from sequoia_pub_amd.pipeline import SlidePipeline  # noqa: E402
from sequoia_pub_amd.uni import UniViT  # noqa: E402
from sequoia_pub_amd.vis import ViS  # noqa: E402

TINY = dict(embed_dim=128, depth=3, num_heads=2, mlp_ratio=4.0, img_size=80)
LARGE = dict(embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, img_size=224)


def _sd(cfg, scale_ls, seed=3):
    return uni_oracle.init_state_dict(dim=cfg["embed_dim"], depth=cfg["depth"], heads=cfg["num_heads"],
                                      mlp_dim=int(cfg["embed_dim"] * cfg["mlp_ratio"]), img_size=cfg["img_size"], seed=seed,
                                      scale_ls=scale_ls)


def _net(mode, cfg, sd):
    m = UniViT(compute_dtype=mode, **cfg)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def large():
    """ViT-L/16 at 224 px with LayerScale gains of O(0.3) (as test_gpu_uni.py), in both parity modes."""
    _lib.require_gpu()
    sd = _sd(LARGE, 0.3)
    return sd, {mode: _net(mode, LARGE, sd) for mode in ("f16x3", "fp32")}


def test_tiny_config_matches_oracle():
    _lib.require_gpu()
    sd = _sd(TINY, 0.5)
    m = _net("f16x3", TINY, sd)
    patches = np.random.RandomState(0).randint(0, 256, (5, 80, 80, 3), dtype=np.uint8)
    got = m.extract_patches_u8(patches).cpu().numpy()
    with torch.no_grad():
        ref = uni_oracle.forward(sd, uni_oracle.transform_patch_u8(patches), heads=2).numpy()
    e = rel_err(got, ref)
    print(f"UNI tiny f16x3: rel err {e:.3e}")
    assert got.shape == (5, 128) and e < 1e-4
    assert rel_err(m(uni_oracle.transform_patch_u8(patches)).cpu().numpy(), got) < 1e-6     # the normalised-tensor call form


def test_vit_large_is_as_close_to_the_exact_features_as_the_reference_is(large):
    """Truth = the oracle in float64 on CPU.  The reference arithmetic (the oracle in fp32) is d_ref from it; the split mode
    must stay within 4 d_ref (the bar of test_gpu_pipeline.py's test_modes_are_as_close_to_the_exact_features_as_the_reference_is)
    and within 1e-4 of the fp32 oracle.  The exact-fp32 MFMA mode of this embedder measured 2.7 d_ref here (2.29e-6 against
    8.4e-7; the split mode 1.56e-6): it is held to the same 4 d_ref, not the ResNet-50 embedder's 2 d_ref."""
    sd, nets = large
    patches = synth.patches_u8(17, n_patches=4, size=224)
    x = uni_oracle.transform_patch_u8(patches)
    torch.set_num_threads(min(16, torch.get_num_threads() or 8))
    with torch.no_grad():
        truth = uni_oracle.forward({k: v.double() for k, v in sd.items()}, x.double(), heads=16).numpy()
        ref32 = uni_oracle.forward(sd, x, heads=16).numpy()
    d_ref = rel_err(ref32, truth)
    got = {mode: nets[mode].extract_patches_u8(patches).cpu().numpy() for mode in ("f16x3", "fp32")}
    d = {mode: rel_err(got[mode], truth) for mode in got}
    d_oracle = rel_err(got["f16x3"], ref32)
    print(f"UNI ViT-L/16 vs exact (fp64) features: reference fp32 {d_ref:.2e}, f16x3 {d['f16x3']:.2e}, fp32 HIP {d['fp32']:.2e}; "
          f"f16x3 vs the fp32 oracle {d_oracle:.2e}")
    assert np.isfinite(got["f16x3"]).all()
    assert d["f16x3"] <= 4.0 * d_ref and d["fp32"] <= 4.0 * d_ref
    assert d_oracle < 1e-4


def test_kmeans_labels_equal_the_fp32_mode(large):
    """One 1000-patch structured slide: k-Means(100) on the split mode's features gives the fp32 mode's labels, 1000 / 1000."""
    _, nets = large
    patches = torch.from_numpy(synth.structured_patches_u8(3, 1000, 224)).cuda()
    f = {mode: nets[mode].extract_patches_u8(patches, sub_batch=500) for mode in ("f16x3", "fp32")}
    r = {mode: kmeans_fit_batch(f[mode].unsqueeze(0), 100) for mode in f}
    same = int((r["f16x3"]["labels"] == r["fp32"]["labels"]).sum())
    e = rel_err(r["f16x3"]["cluster_features"].cpu().numpy(), r["fp32"]["cluster_features"].cpu().numpy())
    print(f"UNI f16x3 vs fp32 on a 1000-patch slide: {same}/1000 labels equal, features {rel_err(f['f16x3'].cpu().numpy(), f['fp32'].cpu().numpy()):.2e}, "
          f"cluster features {e:.2e}")
    assert same == 1000 and e < 1e-4


def test_launch_group_size_does_not_change_the_bits(large):
    _, nets = large
    patches = torch.from_numpy(synth.structured_patches_u8(5, 9, 224)).cuda()
    a = nets["f16x3"].extract_patches_u8(patches, sub_batch=7)
    b = nets["f16x3"].extract_patches_u8(patches, sub_batch=256)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("block", [0, 2])
def test_fp16_overflow_is_detected_and_rerun_in_fp32(block):
    """One fc1 bias pushed past fp16's range (an early block, and the last block whose MLP runs on the class rows only):
    'defer' raises the flag and returns non-finite features, 'raise' raises, the default re-runs in exact fp32."""
    _lib.require_gpu()
    sd = _sd(TINY, 0.5)
    key = f"blocks.{block}.mlp.fc1.bias"
    sd[key] = sd[key].clone()
    sd[key][7] = 7.0e4                                  # GELU(7e4 + ...) > 65504: the hi plane is inf
    nets = {mode: _net(mode, TINY, sd) for mode in ("f16x3", "fp32")}
    patches = torch.from_numpy(synth.structured_patches_u8(1, 12, 80)).cuda()
    exact = nets["fp32"].extract_patches_u8(patches)
    assert torch.isfinite(exact).all()
    flag = nets["f16x3"].new_flag()
    raw = nets["f16x3"].extract_patches_u8(patches, on_nonfinite="defer", flag=flag)
    assert int(flag.item()) == 1 and not torch.isfinite(raw).all()
    with pytest.raises(_lib.SequoiaHipError, match="65504"):
        nets["f16x3"].extract_patches_u8(patches, on_nonfinite="raise")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = nets["f16x3"].extract_patches_u8(patches)
    assert any("fp16" in str(x.message) for x in w)
    assert torch.equal(got, exact)
    healthy = _net("f16x3", TINY, _sd(TINY, 0.5))
    flag = healthy.new_flag()
    ok = healthy.extract_patches_u8(patches, on_nonfinite="defer", flag=flag)
    assert int(flag.item()) == 0 and torch.isfinite(ok).all()


def test_exact_twin_follows_parameter_updates():
    """The fp32 twin that overflowing launch groups re-run in is refreshed when the parameters change."""
    _lib.require_gpu()
    patches = torch.from_numpy(synth.structured_patches_u8(4, 6, 80)).cuda()
    m = None
    for seed in (3, 4):
        sd = _sd(TINY, 0.5, seed=seed)
        sd["blocks.0.mlp.fc1.bias"] = sd["blocks.0.mlp.fc1.bias"].clone()
        sd["blocks.0.mlp.fc1.bias"][1] = 7.0e4
        if m is None:
            m = _net("f16x3", TINY, sd)
        else:
            m.load_state_dict(sd)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = m.extract_patches_u8(patches)
        assert torch.equal(got, _net("fp32", TINY, sd).extract_patches_u8(patches)), seed


def test_pipeline_reembeds_overflowing_slides_in_fp32():
    _lib.require_gpu()
    sd = _sd(TINY, 0.5)
    sd["blocks.1.mlp.fc1.bias"] = sd["blocks.1.mlp.fc1.bias"].clone()
    sd["blocks.1.mlp.fc1.bias"][3] = 7.0e4
    nets = {mode: _net(mode, TINY, sd) for mode in ("f16x3", "fp32")}
    torch.manual_seed(5)
    vis = ViS(num_outputs=50, input_dim=128, depth=1, nheads=2, dimensions_f=64, dimensions_s=64, dimensions_c=64, num_clusters=8,
              device="cuda:0", compute_dtype="fp32").to("cuda:0").eval()
    slides = [torch.from_numpy(synth.structured_patches_u8(i, 40, 80)).cuda() for i in (7, 8)]
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        pipe = SlidePipeline(nets["f16x3"], vis, n_clusters=8, sub_batch=128)
        out = pipe(slides)
        torch.cuda.synchronize()
    ref = SlidePipeline(nets["fp32"], vis, n_clusters=8, sub_batch=128)(slides)
    torch.cuda.synchronize()
    assert pipe.nonfinite_reruns == 2
    assert all(torch.equal(a, b) for a, b in zip(out["labels"], ref["labels"])) and torch.equal(out["pred"], ref["pred"])


def test_compute_features_cli_uni_f16x3(tmp_path, monkeypatch):
    import pandas as pd
    from sequoia_pub_amd.cli import compute_features
    _lib.require_gpu()
    monkeypatch.setenv("SEQUOIA_ALLOW_RANDOM_UNI", "1")
    root = str(tmp_path)
    slide = "TCGA-AA-0000"
    d = os.path.join(root, "patches", slide)
    os.makedirs(d)
    rs = np.random.RandomState(2)
    f = store.File(os.path.join(d, slide + ".hdf5"), "w")
    for t in range(6):
        f.create_dataset(f"{t}_{t + 1}", data=rs.randint(0, 256, (224, 224, 3), dtype=np.uint8))
    f.close()
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name=slide, patient_id="P0", tcga_project="TCGA-BRCA", rna_G0=1.0)]).to_csv(ref, index=False)
    feats = {}
    for mode in ("fp32", "f16x3"):
        out = os.path.join(root, "features_" + mode)
        compute_features.main(["--feat_type", "uni", "--compute_dtype", mode, "--ref_file", ref, "--patch_data_path",
                               os.path.join(root, "patches"), "--feature_path", out])
        h = store.File(os.path.join(out, "TCGA-BRCA", slide, slide + ".h5"), "r")
        feats[mode] = np.asarray(h["uni_features"][:])
        h.close()
    assert feats["f16x3"].shape == (6, 1024)
    e = rel_err(feats["f16x3"], feats["fp32"])
    print(f"compute_features --feat_type uni: f16x3 vs fp32 {e:.2e}")
    assert e < 1e-4
