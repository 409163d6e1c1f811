"""ResNet-50 embedding of rectangular and odd-sized patches (sq_resnet50_extract_hw) against the reference's features
(tests/golden/resnet50_rect.npz: the visualisation path's 256 x 265 tiles, spatial_vis/visualize.py:212-216, and crops at
the corners of the admitted range) in all four modes, at the tolerances the square sizes are held to
(test_gpu_resnet.py: fp32 1e-4, bf16 5e-2; test_gpu_x3.py: bf16x3 1e-4, f16x3 1e-5)."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from gpu_util import rel_err

pytestmark = pytest.mark.gpu

from oracle import resnet_oracle as ro  # noqa: E402  (checker only)
from sequoia_pub_amd import _lib, imgproc, synth  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

SHAPES = ((250, 250), (225, 300), (300, 225), (193, 193), (193, 416), (416, 193), (416, 416), (288, 224))   # make_resnet_rect_golden.py
CROP_SEED0, VIS_SEED = 20, 5
TOL = {"fp32": 1e-4, "bf16": 5e-2, "bf16x3": 1e-4, "f16x3": 1e-5}
MODES = ["fp32", "bf16", "bf16x3", "f16x3"]
X3_SWITCHES = ("SQ_RESNET_NO_TAIL", "SQ_RESNET_NO_CHAIN_DS", "SQ_RESNET_NO_CHAIN", "SQ_RESNET_NO_DUAL", "SQ_RESNET_NO_CHAINW", "SQ_RESNET_NO_STEM_REDUCE")


def _model(mode):
    sd = ro.init_resnet50_state_dict(seed=99, perturb_bn=True)
    m = resnet50(pretrained=False, compute_dtype=mode)
    full = m.state_dict()
    full.update(sd)
    m.load_state_dict(full)
    return m.to("cuda:0").eval(), sd


def crop(i):
    H, W = SHAPES[i]
    return np.ascontiguousarray(synth.patches_u8(CROP_SEED0 + i, n_patches=1, size=416)[:, :H, :W])


def rect(seed, n, H, W):
    """n noise patches of H x W (a crop of a square synthetic slide)."""
    return torch.from_numpy(np.ascontiguousarray(synth.patches_u8(seed, n, max(H, W))[:, :H, :W])).cuda()


def call_hw(m, H, W, patches_u8=None, x_f32=None, entry="hw"):
    """The C entry itself (resnet.py routes multiples of 32 to the square entry): returns (rc, features); the feature buffer
    starts as NaN so that a refused call can be seen to have written nothing."""
    L = _lib.lib()
    w, b = m._pack()
    src = patches_u8 if patches_u8 is not None else x_f32
    n = src.shape[0]
    feats = torch.full((n, 2048), float("nan"), dtype=torch.float32, device="cuda:0")
    need = L.sq_resnet50_workspace_bytes_hw(m.compute_dtype, n, H, W) if entry == "hw" else L.sq_resnet50_workspace_bytes(m.compute_dtype, n, H)
    ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    with torch.cuda.device(0):
        if entry == "hw":
            rc = L.sq_resnet50_extract_hw(m.compute_dtype, _lib.ptr(w), _lib.ptr(b), _lib.ptr(patches_u8), _lib.ptr(x_f32), n, H, W,
                                          _lib.ptr(feats), _lib.ptr(ws), ws.numel(), _lib.ptr(flag), _lib.stream_ptr("cuda:0"))
        else:
            rc = L.sq_resnet50_extract_checked(m.compute_dtype, _lib.ptr(w), _lib.ptr(b), _lib.ptr(patches_u8), _lib.ptr(x_f32), n, H,
                                               _lib.ptr(feats), _lib.ptr(ws), ws.numel(), _lib.ptr(flag), _lib.stream_ptr("cuda:0"))
    torch.cuda.synchronize()
    return rc, feats


@pytest.mark.parametrize("mode", MODES)
def test_features_match_reference_at_every_fixture_shape(golden_dir, mode):
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "resnet50_rect.npz"))
    m, sd = _model(mode)
    tol = TOL[mode]
    errs = {}
    f = m.extract_patches_u8(torch.from_numpy(z["vis_u8"]).cuda()).cpu().numpy()
    assert f.shape == (2, 2048)
    errs["256x265 (visualisation tiles)"] = rel_err(f, z["vis_feat"])
    for i, (H, W) in enumerate(SHAPES):
        f = m.extract_patches_u8(torch.from_numpy(crop(i)).cuda()).cpu().numpy()
        assert f.shape == (1, 2048) and np.isfinite(f).all(), (H, W)
        errs[f"{H}x{W}"] = rel_err(f, z[f"feat_{H}x{W}"])
    for k, e in errs.items():
        print(f"resnet50 {mode} {k}: rel err vs reference {e:.3e} (tolerance {tol:g})")
    assert getattr(m, "last_nonfinite_reruns", 0) == 0           # f16x3 ran as f16x3: no exact-fp32 rerun stood in for it
    bad = {k: e for k, e in errs.items() if not e < tol}
    assert not bad, (mode, bad)


@pytest.mark.parametrize("mode", MODES)
def test_float_input_equals_uint8_input(mode):
    """The reference's call form (normalised fp32 NCHW) against the fused uint8 path at rectangular shapes, as
    test_gpu_resnet.py does at 224.  Both forms evaluate the reference's fp32 transform; a last-bit difference between the host's
    and the device's division can move one bf16 operand by an ulp, so bf16 is held to its mode tolerance and the others to 1e-6."""
    _lib.require_gpu()
    m, sd = _model(mode)
    for H, W in ((256, 265), (193, 416), (250, 250)):
        p = rect(31, 3, H, W)
        fused = m.extract_patches_u8(p).cpu().numpy()
        direct = m.forward_extract(ro.transform_patch_u8(p.cpu())).cpu().numpy()
        e = rel_err(direct, fused)
        print(f"resnet50 {mode} {H}x{W}: fp32 NCHW input vs uint8 input {e:.3e}")
        assert e < (TOL["bf16"] if mode == "bf16" else 1e-6), (H, W, e)


@pytest.mark.parametrize("mode", MODES)
def test_new_entry_is_bit_identical_to_the_square_entry(mode):
    _lib.require_gpu()
    m, sd = _model(mode)
    for S in (224, 256):
        p = torch.from_numpy(synth.patches_u8(40 + S, 3, S)).cuda()
        rc_old, old = call_hw(m, S, S, patches_u8=p, entry="square")
        rc_new, new = call_hw(m, S, S, patches_u8=p, entry="hw")
        assert rc_old == 0 and rc_new == 0, _lib.lib().sq_last_error()
        assert torch.isfinite(old).all()
        assert torch.equal(old, new), (S, float((old - new).abs().max()))
        assert torch.equal(old, m.extract_patches_u8(p))
        x = ro.transform_patch_u8(p.cpu()).cuda().contiguous()
        rc_old, old = call_hw(m, S, S, x_f32=x, entry="square")
        rc_new, new = call_hw(m, S, S, x_f32=x, entry="hw")
        assert rc_old == 0 and rc_new == 0 and torch.equal(old, new), S


@pytest.mark.parametrize("mode", MODES)
def test_batch_and_sub_batch_consistency_at_256x265(mode):
    """A batch of 5 == five single-tile calls == sub_batch=2 chunks (two chains in flight), same bits."""
    _lib.require_gpu()
    m, sd = _model(mode)
    p = rect(3, 5, 256, 265)
    whole = m.extract_patches_u8(p)
    singles = torch.cat([m.extract_patches_u8(p[i:i + 1]) for i in range(5)])
    chunks = m.extract_patches_u8(p, sub_batch=2)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, singles) and torch.equal(whole, chunks)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_x3_fused_routes_are_bit_identical_at_rectangular_shapes(monkeypatch, mode):
    """The twin of test_gpu_x3.py::test_resnet50_x3_fused_chain_is_bit_identical at 256 x 265 (64 x 67 maps: the WIDE tail form
    with H != W) and at 300 x 225 (75 x 57 maps: the narrow tail form with H != W): every fused route against the plain one."""
    _lib.require_gpu()
    m, sd = _model(mode)
    pa, pb = rect(5, 3, 256, 265), rect(6, 2, 300, 225)
    outs = {}
    for tag, env in (("tail", {}), ("no_chainw", {"SQ_RESNET_NO_CHAINW": "1"}), ("no_stem_reduce", {"SQ_RESNET_NO_STEM_REDUCE": "1"}),
                     ("chain", {"SQ_RESNET_NO_TAIL": "1"}), ("chain_no_ds", {"SQ_RESNET_NO_TAIL": "1", "SQ_RESNET_NO_CHAIN_DS": "1"}),
                     ("no_dual", {"SQ_RESNET_NO_DUAL": "1"}), ("dual_everywhere", {"SQ_RESNET_NO_CHAIN": "1"}),
                     ("plain", {"SQ_RESNET_NO_CHAIN": "1", "SQ_RESNET_NO_DUAL": "1", "SQ_RESNET_NO_CHAINW": "1", "SQ_RESNET_NO_STEM_REDUCE": "1"})):
        for k in X3_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        outs[tag] = (m.extract_patches_u8(pa), m.extract_patches_u8(pb))
    torch.cuda.synchronize()
    for k in X3_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert torch.isfinite(outs["tail"][0]).all() and torch.isfinite(outs["tail"][1]).all()
    for tag in ("tail", "no_chainw", "no_stem_reduce", "chain", "chain_no_ds", "no_dual", "dual_everywhere"):
        for j, name in enumerate(("256x265", "300x225")):
            assert torch.equal(outs[tag][j], outs["plain"][j]), (tag, name, float((outs[tag][j] - outs["plain"][j]).abs().max()))


def test_bf16_fused_routes_are_bit_identical_at_rectangular_shapes(monkeypatch):
    """The twin of test_gpu_resnet.py::test_fused_bottleneck_tail_is_bit_identical: SQ_RESNET_NO_FUSE=1 against the default at
    256 x 265 (67-wide maps do not fit the 56 x 56 tail's halo: the row-wise chains only) and at 300 x 225 (75 x 57 maps: the tail
    with H != W)."""
    _lib.require_gpu()
    m, sd = _model("bf16")
    for H, W, n in ((256, 265, 3), (300, 225, 1), (300, 225, 3)):
        p = rect(11 + n, n, H, W)
        monkeypatch.delenv("SQ_RESNET_NO_FUSE", raising=False)
        fused = m.extract_patches_u8(p)
        monkeypatch.setenv("SQ_RESNET_NO_FUSE", "1")
        plain = m.extract_patches_u8(p)
        torch.cuda.synchronize()
        assert torch.isfinite(fused).all()
        assert torch.equal(fused, plain), (H, W, n, float((fused - plain).abs().max()))
    monkeypatch.delenv("SQ_RESNET_NO_FUSE", raising=False)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_x3_halo_staged_3x3_at_256x265(golden_dir, mode):
    """conv_halo_x3.hip takes the 32 x 34, 16 x 17 and 8 x 9 maps of a 256 x 265 tile; the implicit-GEMM form (sq_dbg_set key 8 = 0)
    walks K in another order, so the two are not bit-equal: each is held to the mode's tolerance against the reference, and
    therefore (triangle inequality) to twice that against each other."""
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "resnet50_rect.npz"))
    lib = _lib.lib()
    m, sd = _model(mode)
    p = torch.from_numpy(z["vis_u8"]).cuda()
    outs = {}
    try:
        for halo in (-1, 0):
            lib.sq_dbg_set(8, halo)
            outs[halo] = m.extract_patches_u8(p).cpu().numpy()
    finally:
        lib.sq_dbg_set(8, -1)
    e_on, e_off, e_mut = rel_err(outs[-1], z["vis_feat"]), rel_err(outs[0], z["vis_feat"]), rel_err(outs[-1], outs[0])
    print(f"resnet50 {mode} 256x265: halo-staged 3x3 {e_on:.3e}, implicit GEMM {e_off:.3e} vs reference; against each other {e_mut:.3e}")
    assert e_on < TOL[mode] and e_off < TOL[mode] and e_mut < 2 * TOL[mode]


def test_bf16_halo_staged_3x3_at_256x265():
    """The twin of test_gpu_resnet.py::test_halo_staged_3x3_matches_implicit_gemm on 256 x 265 tiles (16 x 17 and 8 x 9 maps)."""
    _lib.require_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for halo in ("1", "0"):                       # the switch is read once per process
        env = dict(os.environ, SQ_CONV_HALO=halo, SQ_CONV_HALO_MIN_TILES="1")
        path = os.path.join("/tmp", f"sq_rect_halo_{halo}_{os.getpid()}.pt")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "rect_halo_worker.py"), path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-800:]
        outs.append(torch.load(path))
        os.remove(path)
    a, b = outs
    assert torch.isfinite(a).all() and not torch.equal(a, b)            # a different kernel really ran
    assert float((a - b).abs().max() / b.abs().max()) < 1e-2


@pytest.mark.parametrize("mode", MODES)
def test_sizes_outside_the_range_are_refused(mode):
    """(192, 256), (256, 417) and a 448-square through the new entry: an error that says why, nothing launched (the NaN-filled
    feature buffer is untouched); resnet.py turns the first two into a ValueError naming the range."""
    _lib.require_gpu()
    m, sd = _model(mode)
    for H, W in ((192, 256), (256, 417), (448, 448)):
        p = torch.zeros(1, H, W, 3, dtype=torch.uint8, device="cuda:0")
        assert _lib.lib().sq_resnet50_workspace_bytes_hw(m.compute_dtype, 1, H, W) == 0
        rc, feats = call_hw(m, H, W, patches_u8=p)
        msg = _lib.lib().sq_last_error().decode()
        assert rc != 0 and "193" in msg and "416" in msg and f"{H} x {W}" in msg, (rc, msg)
        assert bool(torch.isnan(feats).all())
    for H, W in ((192, 256), (256, 417)):
        with pytest.raises(ValueError, match=r"\[193, 416\]"):
            m.extract_patches_u8(torch.zeros(1, H, W, 3, dtype=torch.uint8, device="cuda:0"))
        with pytest.raises(ValueError, match=r"\[193, 416\]"):
            m.forward_extract(torch.zeros(1, 3, H, W, device="cuda:0"))


def test_f16x3_overflow_rerun_at_256x265():
    """An activation beyond fp16's range at a rectangular shape: the flag is raised and the exact-fp32 rerun gives fp32's features."""
    _lib.require_gpu()
    sd = ro.init_resnet50_state_dict(seed=99, perturb_bn=True)
    sd["layer1.0.bn3.weight"] = sd["layer1.0.bn3.weight"] * 3.0e4       # as test_gpu_pipeline.py's overflow test
    nets = {}
    for mode in ("f16x3", "fp32"):
        net = resnet50(pretrained=False, compute_dtype=mode)
        full = net.state_dict()
        full.update(sd)
        net.load_state_dict(full)
        nets[mode] = net.to("cuda:0").eval()
    m, ref = nets["f16x3"], nets["fp32"]
    p = rect(9, 2, 256, 265)
    with pytest.raises(_lib.SequoiaHipError):
        m.extract_patches_u8(p, on_nonfinite="raise")
    with pytest.warns(RuntimeWarning):
        got = m.extract_patches_u8(p)
    want = ref.extract_patches_u8(p)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    with pytest.warns(RuntimeWarning):
        got_f = m.forward_extract(ro.transform_patch_u8(p.cpu()))
    assert torch.isfinite(got_f).all() and rel_err(got_f.cpu().numpy(), want.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("mode", MODES)
def test_embed_tiles_rectangular_out_size(golden_dir, mode):
    """visualize.embed_tiles(out_size=(256, 265), resize="pil"): at 20x the 256-pixel tiles become the fixture's Pillow-resized
    tiles byte for byte and their features sit within the mode's tolerance of the oracle on those; at 40x 512-pixel tiles go
    to 256 x 265 in the same call."""
    from sequoia_pub_amd.cli.visualize import embed_tiles
    from sequoia_pub_amd.patchgen import ArraySlide
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "resnet50_rect.npz"))
    m, sd = _model(mode)
    p256 = synth.patches_u8(VIS_SEED, n_patches=2, size=256)
    slide = ArraySlide([np.concatenate([p256[0], p256[1]], axis=1)])                    # two tiles side by side
    df = pd.DataFrame([(0, 0), (256, 0)], columns=["xcoord", "ycoord"])
    resized = imgproc.resize_u8_pil(torch.from_numpy(p256).cuda(), (256, 265), "bilinear")
    assert resized.shape == (2, 256, 265, 3) and np.array_equal(resized.cpu().numpy(), z["vis_u8"])
    got = embed_tiles(slide, df, 256, (256, 265), m, "cuda:0", resize="pil")
    assert got.shape == (2, 2048)
    assert torch.equal(got, m.extract_patches_u8(resized))
    torch.set_num_threads(8)
    oracle = ro.embed_patches(sd, z["vis_u8"], batch=1).numpy()
    e = rel_err(got.cpu().numpy(), oracle)
    print(f"embed_tiles {mode} 20x, 256 -> 256x265: rel err vs oracle {e:.3e}")
    assert e < TOL[mode]
    # 40x: tiles of 512
    rng = np.random.default_rng(2)
    slide40 = ArraySlide([rng.integers(0, 256, (600, 1100, 3), dtype=np.uint8)])
    df40 = pd.DataFrame([(0, 0), (512, 0), (300, 44)], columns=["xcoord", "ycoord"])
    tiles = torch.from_numpy(np.stack([np.asarray(slide40.read_region((x, y), 0, (512, 512)))[..., :3] for x, y in zip(df40.xcoord, df40.ycoord)])).cuda()
    small = imgproc.resize_u8_pil(tiles, (256, 265), "bilinear")
    assert small.shape == (3, 256, 265, 3)
    got40 = embed_tiles(slide40, df40, 512, (256, 265), m, "cuda:0", chunk=2, resize="pil")
    assert got40.shape == (3, 2048) and torch.isfinite(got40).all()
    assert torch.equal(got40[:2], m.extract_patches_u8(small[:2])) and torch.equal(got40[2:], m.extract_patches_u8(small[2:]))
    with pytest.raises(ValueError):
        embed_tiles(slide, df, 256, (256, 265), m, "cuda:0", resize="float")
    # an int and an equal pair mean the same square input
    assert torch.equal(embed_tiles(slide, df, 256, (256, 256), m, "cuda:0"), embed_tiles(slide, df, 256, 256, m, "cuda:0"))


def test_visualize_cli_resnet_input_reference(tmp_path):
    """cli.visualize --resnet_input reference: every tile goes through the 256 x 265 resize (although the slide is 20x and --resize
    says float), the CSV is written, equals the library calls on the 256 x 265 feature cache and differs from the default run's."""
    from sequoia_pub_amd.cli import visualize
    from sequoia_pub_amd.spatial import sliding_window_method
    from sequoia_pub_amd.vis import ViS
    _lib.require_gpu()
    root = str(tmp_path)
    rs = np.random.RandomState(4)
    nx, ny, G = 9, 8, 12                                    # the slide of test_gpu_spatial.py's CLI test: windows are 10 x 10 tiles
    arr = rs.randint(0, 256, ((ny + 1) * 256, (nx + 1) * 256, 3), dtype=np.uint8)
    os.makedirs(os.path.join(root, "TCGA", "P"))
    np.save(os.path.join(root, "TCGA", "P", "TCGA-X.npy"), arr)
    mask = np.ones(((nx + 1) * 8, (ny + 1) * 8), dtype=bool)
    mask[:, 56:] = False                                    # background from tile row 7 on
    np.save(os.path.join(root, "mask.npy"), mask)
    genes = [f"G{i}" for i in range(G)]
    rw = os.path.join(root, "resnet.pth")
    torch.save({**resnet50().state_dict(), **ro.init_resnet50_state_dict(seed=3)}, rw)
    ck = os.path.join(root, "vis_resnet", "st")
    os.makedirs(ck)
    pickle.dump({"genes": genes}, open(os.path.join(ck, "test_results.pkl"), "wb"))
    torch.manual_seed(7)
    torch.save(ViS(G, 2048, 6, 16, 64, 64, 64, device="cpu").state_dict(), os.path.join(ck, "model_best.pt"))
    common = ["--study", "st", "--project", "P", "--gene_names", "G3,G7", "--wsi_file_name", "TCGA-X.npy", "--save_folder", "t",
              "--feat_type", "resnet", "--slide_path", os.path.join(root, "TCGA", "P"), "--mask_path", os.path.join(root, "mask.npy"),
              "--extractor_weights", rw, "--compute_dtype", "fp32", "--model_type", "vis", "--folds", "0", "--checkpoint", ck]
    res_def, path_def = visualize.main(common + ["--out_root", os.path.join(root, "out_default")])
    res_ref, path_ref = visualize.main(common + ["--out_root", os.path.join(root, "out_reference"), "--resnet_input", "reference"])
    assert os.path.basename(path_ref) == "stride-1.csv" and os.path.exists(path_ref) and path_ref != path_def
    back = pd.read_csv(path_ref, index_col=0)
    assert len(back) == len(res_ref) == len(res_def) == nx * (ny - 1) and np.isfinite(back["G3"].values).all()
    assert not np.array_equal(res_ref["G3"].values, res_def["G3"].values)
    # the same numbers from the library on the 256 x 265 cache
    feat_model = resnet50()
    feat_model.load_state_dict(torch.load(rw))
    feat_model = feat_model.to("cuda:0").eval()
    df = visualize.valid_tiles(mask, (arr.shape[1], arr.shape[0]), 256)
    tiles = visualize.read_tiles(visualize.open_slide(os.path.join(root, "TCGA", "P", "TCGA-X.npy")), df, 256)
    cache_ref = feat_model.extract_patches_u8(imgproc.resize_u8_pil(tiles.cuda(), (256, 265), "bilinear"))
    cache_def = feat_model.extract_patches_u8(tiles.cuda())
    assert not torch.equal(cache_ref, cache_def)
    m = ViS(G, 2048, 6, 16, 64, 64, 64, device="cuda:0")
    m.load_state_dict(torch.load(os.path.join(ck, "model_best.pt")))
    m = m.to("cuda:0").eval()
    for res, cache in ((res_ref, cache_ref), (res_def, cache_def)):
        direct = sliding_window_method(df, cache, m, [3], 1)
        np.testing.assert_allclose(res["G3_0"].values, np.array([direct[3][i] for i in res.index]), rtol=1e-5, atol=1e-6)
