"""Sliding-window maps (spatial_vis/visualize.py:35-102) for the two comparator aggregators, --model_type vit and he2rna, through
the gather / vote path of spatial.sliding_window_method: against a literal per-window loop over the oracle models
(oracle.vis_oracle.vit_forward, oracle.he2rna_oracle.forward_eval) and against spatial.sliding_window_any_model; the HE2RNA
window kernel against the kernel on the materialised window batch; rank sharding; the visualize CLI."""
import filecmp
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

from oracle import he2rna_oracle, vis_oracle  # noqa: E402  (checkers only)
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.he2rna import HE2RNA  # noqa: E402
from sequoia_pub_amd.spatial import sliding_window_all_genes, sliding_window_any_model, sliding_window_method  # noqa: E402
from sequoia_pub_amd.vit import ViT  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
KS = [1, 2, 5, 10, 20, 50, 100]


# ---- literal references ------------------------------------------------------------------------------------------------------
def reference_windows(df, stride, probes=None):
    """The kept windows of visualize.py:46-52 in visiting order, as arrays of df index values; with `probes`, only the windows
    that hold one of those tiles."""
    max_x, max_y = max(df['xcoord_tf']), max(df['ycoord_tf'])
    px = None if probes is None else [(int(df['xcoord_tf'][k]), int(df['ycoord_tf'][k])) for k in probes]
    wins = []
    for x in range(0, max_x, stride):
        for y in range(0, max_y, stride):
            if px is not None and not any(x <= tx < x + 10 and y <= ty < y + 10 for tx, ty in px):
                continue
            window = df[((df['xcoord_tf'] >= x) & (df['xcoord_tf'] < (x + 10))) & ((df['ycoord_tf'] >= y) & (df['ycoord_tf'] < (y + 10)))]
            if window.shape[0] > 50:
                wins.append(window.index.values)
    return wins


def window_batch(feats, wins):
    """[len(wins), 100, D]: the window's tile features, zero-padded (visualize.py:72-75)."""
    x = torch.zeros(len(wins), 100, feats.shape[1])
    for j, idx in enumerate(wins):
        x[j, :len(idx)] = feats[idx]
    return x


def oracle_predictions(model_fn, feats, wins, batch=32):
    out = []
    with torch.no_grad():
        for i in range(0, len(wins), batch):
            out.append(model_fn(window_batch(feats, wins[i:i + batch])))
    return torch.cat(out).double().numpy()


def vote(wins, preds, stride, tiles=None):
    """visualize.py:86-101: stride 10 the last writer wins, else the mean over the windows holding the tile (NaN propagates)."""
    per = {}
    for w, idx in enumerate(wins):
        for t in idx:
            if tiles is None or t in tiles:
                per.setdefault(int(t), []).append(w)
    return {t: (preds[ws[-1]] if stride == 10 else np.mean(preds[ws], axis=0)) for t, ws in per.items()}


def vit_fn(sd, heads, literal_2d=False):
    if literal_2d:      # the reference's 2-D [100, D] input: rearrange -> [100, 1, D] + pos_emb1D, prediction = row 0
        return lambda x: torch.stack([vis_oracle.vit_forward(sd, xi[:, None, :], heads)[0] for xi in x])
    return lambda x: vis_oracle.vit_forward(sd, x, heads)


def he2rna_fn(sd, input_dim):
    return lambda x: he2rna_oracle.forward_eval(sd, x.transpose(1, 2), KS, input_dim)       # channels x tiles (visualize.py:79-81)


# ---- models --------------------------------------------------------------------------------------------------------------------
def make_vit(seed, mode, **cfg):
    torch.manual_seed(seed)
    m = ViT(**cfg, device="cuda:0", compute_dtype=mode)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:                                         # non-trivial LayerNorm parameters
        if k.endswith(("norm.weight", "net.0.weight", "linear_head.0.weight")):
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith(("norm.bias", "net.0.bias", "linear_head.0.bias")):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=g)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval(), sd


def make_he2rna(seed, input_dim, G):
    torch.manual_seed(seed)
    m = HE2RNA(input_dim=input_dim, output_dim=G, layers=[256, 256], ks=KS, device="cpu")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.to("cuda:0")
    m.device = "cuda:0"
    return m.eval(), sd


def relu_features(rs, n, D, zero_frac):
    """ResNet-like (post-ReLU) tile features; a share of all-zero tiles (mask 0, he2rna.py:94-95)."""
    f = np.maximum(rs.randn(n, D), 0).astype(np.float32)
    f[rs.rand(n) < zero_frac] = 0
    return torch.from_numpy(f)


def holey_grid(seed, nx, ny, keep=0.75):
    rs = np.random.RandomState(seed)
    coords = [(x, y) for x in range(nx) for y in range(ny) if rs.rand() < keep]
    return pd.DataFrame(coords, columns=["xcoord_tf", "ycoord_tf"]), rs


def check_all_genes(out, votes, ref, G, tol):
    out, votes = out.cpu().numpy(), votes.cpu().numpy()
    covered = sorted(ref)
    assert set(np.nonzero(votes > 0)[0]) == set(covered) and len(covered) > 0
    assert np.isnan(out[votes == 0]).all()
    b = np.stack([ref[k] for k in covered])
    a = out[covered]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    assert rel_err(a[fin], b[fin]) < tol
    return a, b


def check_dict(got, ref, genes, tol):
    for g in genes:
        assert set(got[g].keys()) == set(ref) and len(ref) > 0
        a = np.array([got[g][k] for k in sorted(ref)], dtype=np.float64)
        b = np.array([ref[k][g] for k in sorted(ref)], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert rel_err(a[~np.isnan(b)], b[~np.isnan(b)]) < tol


# ---- 1. ViT vs the literal loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,literal", [(10, False), (2, False), (1, False), (5, True)])
def test_vit_sliding_window_matches_literal_loop(stride, literal):
    _lib.require_gpu()
    df, rs = holey_grid(1, 23, 19)
    feats = torch.from_numpy(rs.randn(len(df), 128).astype(np.float32))
    m, sd = make_vit(3, "fp32", num_outputs=37, dim=128, depth=2, heads=2, mlp_dim=256)       # G = 37: the scalar vote path
    wins = reference_windows(df, stride)
    ref = vote(wins, oracle_predictions(vit_fn(sd, 2, literal), feats, wins), stride)
    out, votes = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats, m, stride, literal_2d=literal, batch_windows=29)
    check_all_genes(out, votes, ref, 37, 1e-4)
    genes = [0, 11, 36]
    got = sliding_window_method(df, feats, m, genes, stride, literal_2d=literal, batch_windows=29)
    check_dict(got, ref, genes, 1e-4)


# ---- 2. HE2RNA window kernel == the kernel on the materialised batch ----------------------------------------------------------
def window_kernel(scores, mask, idx, G):
    ks = np.asarray(KS, dtype=np.int32)
    out = torch.empty(idx.shape[0], G, device="cuda:0")
    _lib.check(_lib.lib().sq_he2rna_window_topk_mean(_lib.ptr(scores), scores.shape[1], _lib.ptr(mask), scores.shape[0], _lib.ptr(idx),
                                                     ks.ctypes.data, len(ks), 1.0 / len(ks), _lib.ptr(out), idx.shape[0], idx.shape[1], G,
                                                     _lib.stream_ptr(scores.device)))
    return out


def materialised_kernel(scores, mask, idx, G):
    ok = (idx >= 0) & (idx < scores.shape[0])
    safe = torch.where(ok, idx, 0).long()
    s = torch.where(ok[..., None], scores[safe], 0.0).contiguous()                       # [W, N, ld]
    w = torch.where(ok, mask[safe], 0.0).contiguous()
    ks = np.asarray(KS, dtype=np.int32)
    out = torch.empty(idx.shape[0], G, device="cuda:0")
    _lib.check(_lib.lib().sq_he2rna_topk_mean(_lib.ptr(s), s.shape[2], _lib.ptr(w), ks.ctypes.data, len(ks), 1.0 / len(ks), _lib.ptr(out),
                                              idx.shape[0], idx.shape[1], G, _lib.stream_ptr(scores.device)))
    return out


@pytest.mark.parametrize("G,W", [(300, 900), (37, 65600)], ids=["G300", "G37_over_65535_windows"])
def test_he2rna_window_kernel_is_bit_equal_to_the_materialised_kernel(G, W):
    _lib.require_gpu()
    g = torch.Generator().manual_seed(G)
    rows = 5000
    ld = (G + 7) // 8 * 8
    scores = (torch.randint(-6, 7, (rows, ld), generator=g).float() * 0.25).cuda()        # coarse values: many ties
    mask = (torch.rand(rows, generator=g) > 0.2).float().cuda()
    idx = torch.randint(0, rows, (W, 100), generator=g, dtype=torch.int32)
    n_valid = torch.randint(51, 101, (W,), generator=g)
    idx[torch.arange(100)[None, :] >= n_valid[:, None]] = -1                            # -1 padding behind the tiles
    dead = torch.nonzero(mask.cpu() == 0).ravel()
    idx[::7, :5] = dead[torch.randint(0, dead.numel(), (idx[::7].shape[0], 5), generator=g)].to(torch.int32)   # first k slots masked -> NaN
    idx[3::11, 60] = rows + 17                                                          # out of range: the zero padding
    idx = idx.cuda().contiguous()
    a = window_kernel(scores, mask, idx, G)
    b = materialised_kernel(scores, mask, idx, G)
    torch.cuda.synchronize()
    assert bool(torch.isnan(a).any()) and bool(torch.isfinite(a).any())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))                        # NaN positions included


# ---- 3. HE2RNA vs the literal loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [10, 2])
def test_he2rna_sliding_window_matches_literal_loop(stride):
    _lib.require_gpu()
    df, rs = holey_grid(7, 24, 21)
    feats = relu_features(rs, len(df), 64, 0.04)
    feats[0] = 0                                 # the first tile of window (0, 0) is masked: its k = 1 mean is 0/0 = NaN
    m, sd = make_he2rna(8, 64, 37)
    wins = reference_windows(df, stride)
    ref = vote(wins, oracle_predictions(he2rna_fn(sd, 64), feats, wins), stride)
    out, votes = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats, m, stride)
    a, b = check_all_genes(out, votes, ref, 37, 1e-4)
    assert np.isnan(b).any() and (~np.isnan(b)).any()              # the first-k-positions quirk is exercised
    genes = [0, 5, 36]
    got = sliding_window_method(df, feats, m, genes, stride)
    check_dict(got, ref, genes, 1e-4)
    lit = sliding_window_any_model(df, feats, m, genes, stride, "he2rna")
    check_dict(got, {k: {g: lit[g][k] for g in genes} for k in lit[genes[0]]}, genes, 1e-4)
    with pytest.raises(ValueError):
        sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats, m, stride, literal_2d=True)


# ---- 4. real size, 40 x 30 grid, probe tiles ------------------------------------------------------------------------------------
def probe_check(out, votes, df, feats, fn, probes, tol, label):
    wins = reference_windows(df, 1, probes)
    preds = oracle_predictions(fn, feats, wins, batch=8)
    ref = vote(wins, preds, 1, tiles=set(probes))
    errs = {k: rel_err(out[k].cpu().numpy(), ref[k]) for k in probes}
    print(f"{label}: {len(wins)} oracle windows, votes {[int(votes[k]) for k in probes]}, worst rel err {max(errs.values()):.2e}")
    assert max(errs.values()) < tol, errs


def test_real_size_40x30_probe_tiles():
    """The models at the size visualize.py builds them (ViT dim 2048, depth 6, 16 heads, mlp 2048; HE2RNA [256, 256]), G = 20 820,
    stride 1; probe tiles -- corners, edges, interior, 1 ... 100 windows -- against the literal loop over the oracle models."""
    _lib.require_gpu()
    nx, ny = 40, 30
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    df = pd.DataFrame({"xcoord_tf": xs.ravel(), "ycoord_tf": ys.ravel()})
    at = lambda x, y: x * ny + y
    feats = relu_features(np.random.RandomState(11), nx * ny, 2048, 0.0)
    cfg = dict(num_outputs=20820, dim=2048, depth=6, heads=16, mlp_dim=2048)
    probes = [at(0, 0), at(39, 29), at(20, 15), at(12, 0)]
    wins = reference_windows(df, 1, probes)
    for mode, tol in (("fp32", 1e-4), ("bf16", 3e-2)):
        m, sd = make_vit(12, mode, **cfg)
        out, votes = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats.cuda(), m, 1, batch_windows=512)
        assert out.shape == (nx * ny, 20820) and not bool(torch.isnan(out).any())
        assert int(votes[at(0, 0)]) == 1 and int(votes[at(20, 15)]) == 100
        if mode == "fp32":
            ref = vote(wins, oracle_predictions(vit_fn(sd, 16), feats, wins, batch=8), 1, tiles=set(probes))
        errs = {k: rel_err(out[k].cpu().numpy(), ref[k]) for k in probes}
        print(f"ViT 40 x 30 {mode}: {len(wins)} oracle windows, worst rel err {max(errs.values()):.2e}")
        assert max(errs.values()) < tol, errs
        del m, out
    m, sd = make_he2rna(13, 2048, 20820)
    out, votes = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats.cuda(), m, 1)
    probe_check(out, votes, df, feats, he2rna_fn(sd, 2048), probes + [at(3, 27), at(39, 4)], 1e-4, "HE2RNA 40 x 30 fp32")


# ---- 5. BASELINE config 5 as stated: 250 x 200 = 50 000 tiles, stride 1 --------------------------------------------------------------
@pytest.mark.parametrize("model_type", ["vit", "he2rna"])
def test_config5_full_size_probe_tiles_and_batch_invariance(model_type):
    _lib.require_gpu()
    nx, ny = 250, 200
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    df = pd.DataFrame({"xcoord_tf": xs.ravel(), "ycoord_tf": ys.ravel()})
    at = lambda x, y: x * ny + y
    feats = relu_features(np.random.RandomState(21), nx * ny, 1024, 0.0)
    if model_type == "vit":
        m, sd = make_vit(22, "bf16", num_outputs=20820, dim=1024, depth=6, heads=16, mlp_dim=2048)
        fn, tol = vit_fn(sd, 16), 3e-2
    else:
        m, sd = make_he2rna(22, 1024, 20820)
        fn, tol = he2rna_fn(sd, 1024), 1e-4
    fd = feats.cuda()
    out, votes = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, fd, m, 1, batch_windows=2048)
    assert out.shape == (nx * ny, 20820) and bool(torch.isfinite(out[votes > 0]).all())
    assert int(votes.max()) == 100 and int((votes > 0).sum()) > 49000
    probes = [at(0, 0), at(120, 0), at(131, 97)]
    probe_check(out, votes, df, feats, fn, probes, tol, f"config 5 full size {model_type}")
    out2, votes2 = sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, fd, m, 1, batch_windows=700)
    assert torch.equal(votes, votes2)
    keep = votes > 0
    if model_type == "he2rna":
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    else:
        diff = float((out[keep] - out2[keep]).abs().max() / out[keep].abs().max())
        print(f"  2048 vs 700 windows per forward: max difference {diff:.2e} of max")
        assert diff < 1e-5


# ---- 6. ranks: bit-identical to one rank -----------------------------------------------------------------------------------------
def launch(nproc, worker, args, timeout=900):
    port = 29500 + (os.getpid() * 13 + abs(hash(tuple(map(str, args)))) % 991) % 2000
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SQ_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, worker)] + [str(a) for a in args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0


@pytest.mark.parametrize("case", [
    # model, nx, ny, mode, batch_windows, stride, holes, head_chunk, size, ranks
    ("vit", 250, 200, "bf16", 1024, 1, 0, 4096, "full", 2),
    ("he2rna", 250, 200, "fp32", 1024, 1, 0, 4096, "full", 2),
    ("vit", 23, 17, "fp32", 16, 1, 1, 64, "small", 2),
    ("he2rna", 23, 17, "fp32", 16, 1, 1, 64, "small", 3),
    ("vit", 23, 17, "bf16", 40, 1, 1, 64, "small", 3),
    ("he2rna", 31, 29, "fp32", 2, 10, 1, 4096, "small", 2),
    ("vit", 31, 29, "fp32", 2, 10, 0, 4096, "small", 2),
], ids=["vit_full_size_bf16", "he2rna_full_size", "vit_holes", "he2rna_three_ranks_holes", "vit_three_ranks_bf16",
        "he2rna_stride10_rank1_no_chunk", "vit_stride10_rank1_no_chunk"])
def test_comparator_sharded_slide_is_bit_identical_to_the_one_rank_result(tmp_path, case):
    *args, ranks = case
    launch(ranks, "comparator_multirank_worker.py", [tmp_path] + args)
    assert all((tmp_path / f"ok{r}").read_text() == "ok" for r in range(ranks))


# ---- 7. the visualize CLI ---------------------------------------------------------------------------------------------------------
def test_visualize_cli_vit_and_he2rna(tmp_path):
    """spatial_vis/visualize.py:104-307 with --model_type vit (two folds) and he2rna on a synthetic slide: the CSV columns equal the
    library call on the same feature cache, agree with the literal per-window form, and two ranks write the one-rank CSV."""
    from oracle import resnet_oracle
    from sequoia_pub_amd.cli import visualize
    from sequoia_pub_amd.resnet import resnet50
    _lib.require_gpu()
    root = str(tmp_path)
    rs = np.random.RandomState(4)
    nx, ny, G = 12, 11, 24
    arr = rs.randint(0, 256, ((ny + 1) * 256, (nx + 1) * 256, 3), dtype=np.uint8)
    os.makedirs(os.path.join(root, "TCGA", "P"))
    np.save(os.path.join(root, "TCGA", "P", "TCGA-X.npy"), arr)
    mask = np.ones(((nx + 1) * 8, (ny + 1) * 8), dtype=bool)
    mask[:, 80:] = False                                                                   # background from tile row 10 on
    np.save(os.path.join(root, "mask.npy"), mask)
    genes = [f"G{i}" for i in range(G)]
    rw = os.path.join(root, "resnet.pth")
    torch.save({**resnet50().state_dict(), **resnet_oracle.init_resnet50_state_dict(seed=3)}, rw)
    torch.manual_seed(7)
    for mt in ("vit", "he2rna"):
        ck = os.path.join(root, f"{mt}_resnet", "st")
        os.makedirs(ck)
        pickle.dump({"genes": genes}, open(os.path.join(ck, "test_results.pkl"), "wb"))
        for fold in (0, 1):
            if mt == "vit":
                m = ViT(num_outputs=G, dim=2048, depth=6, heads=16, mlp_dim=2048, device="cpu")
                torch.save(m.state_dict(), os.path.join(ck, "model_best.pt" if fold == 0 else f"model_best_{fold}.pt"))
            else:
                torch.save(HE2RNA(input_dim=2048, layers=[256, 256], ks=KS, output_dim=G), os.path.join(ck, f"model_{fold}.pt"))
    common = ["--study", "st", "--project", "P", "--gene_names", "G3,G17", "--wsi_file_name", "TCGA-X.npy", "--save_folder", "t",
              "--feat_type", "resnet", "--slide_path", os.path.join(root, "TCGA", "P"), "--mask_path", os.path.join(root, "mask.npy"),
              "--extractor_weights", rw, "--compute_dtype", "fp32", "--tile_chunk", "64"]
    feat_model = resnet50()
    feat_model.load_state_dict(torch.load(rw))
    feat_model = feat_model.to("cuda:0").eval()
    df = visualize.valid_tiles(mask, (arr.shape[1], arr.shape[0]), 256)
    cache = feat_model.extract_patches_u8(visualize.read_tiles(visualize.open_slide(os.path.join(root, "TCGA", "P", "TCGA-X.npy")), df, 256).cuda())
    for mt, folds in (("vit", "0,1"), ("he2rna", "1")):
        ck = os.path.join(root, f"{mt}_resnet", "st")
        args = common + ["--model_type", mt, "--folds", folds, "--checkpoint", ck]
        res, p1 = visualize.main(args + ["--out_root", os.path.join(root, f"out1_{mt}")])
        assert len(res) == nx * (ny - 1) and os.path.basename(p1) == "stride-1.csv"
        if mt == "vit":
            m = ViT(num_outputs=G, dim=2048, depth=6, heads=16, mlp_dim=2048, device="cuda:0")
            m.load_state_dict(torch.load(os.path.join(ck, "model_best_1.pt")))
        else:
            m = HE2RNA(input_dim=2048, layers=[256, 256], ks=KS, output_dim=G)
            m.load_state_dict(torch.load(os.path.join(ck, "model_1.pt"), weights_only=False).state_dict())
            m.device = "cuda:0"
        m = m.to("cuda:0").eval()
        direct = sliding_window_method(df, cache, m, [3, 17], 1)
        literal = sliding_window_any_model(df, cache, m, [3, 17], 1, mt)
        for g in (3, 17):
            col = res[f"G{g}_1"].values
            d = np.array([direct[g][i] for i in res.index])
            lit = np.array([literal[g][i] for i in res.index])
            assert np.array_equal(np.isnan(col), np.isnan(d)) and np.array_equal(np.isnan(d), np.isnan(lit))
            ok = ~np.isnan(d)
            assert ok.sum() > 0.9 * len(d)
            assert rel_err(col[ok], d[ok]) < 1e-5
            assert rel_err(d[ok], lit[ok]) < 1e-4
        launch(2, "multirank_worker.py", ["cli", "visualize"] + args + ["--out_root", os.path.join(root, f"out2_{mt}")])
        assert filecmp.cmp(p1, p1.replace(f"out1_{mt}", f"out2_{mt}"), shallow=False), f"{mt}: the two-rank CSV differs from the one-rank CSV"
