"""k-Means of a ragged batch (kmeans_fit_ragged / sq_kmeans_fit_ragged): every slide of a call is bit-equal -- labels,
seeding indices, iteration count, cluster means -- to kmeans_fit of that slide alone, whatever its company and position;
anchored to the scikit-learn goldens (tests/golden/kmeans.npz) and the CPU oracle."""
import filecmp
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import kmeans_oracle as ko  # noqa: E402  (checker only)
from sequoia_pub_amd import _lib, synth  # noqa: E402
from sequoia_pub_amd.kmeans import kmeans_fit, kmeans_fit_batch, kmeans_fit_ragged, ragged_plan  # noqa: E402

COUNTS_64 = [100, 257, 600, 1024, 1025, 2048, 2049, 1000]      # n = k; odd n (no float4 path); both sides of the seeding-class
KINDS_64 = ["gmm", "lowrank", "normal", "gmm", "lowrank", "gmm", "normal", "lowrank"]      # borders 1024 / 2048; (non-)multiples of 64


def alone(X):
    """kmeans_fit of one slide as host arrays (labels, indices, n_iter, cluster_features)."""
    r = kmeans_fit(torch.from_numpy(X).cuda(), 100)
    return (r["labels"][0].cpu().numpy(), r["indices"][0].cpu().numpy(), int(r["n_iter"][0]), r["cluster_features"][0].cpu().numpy())


def slide_of(r, i):
    return (r["labels"][i].cpu().numpy(), r["indices"][i].cpu().numpy(), int(r["n_iter"][i]), r["cluster_features"][i].cpu().numpy())


def same(a, b, equal_nan=False):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            and np.array_equal(a[3], b[3], equal_nan=equal_nan))


def oracle(X):
    """The CPU oracle's fit of one slide, in the form of alone()."""
    o = ko.kmeans_fit(X)
    return (o["labels"], o["indices"], o["n_iter"], ko.cluster_means(X, o["labels"]))


def ragged(Xs, **kw):
    return kmeans_fit_ragged([torch.from_numpy(x).cuda() for x in Xs], 100, **kw)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kmeans.npz"))


@pytest.fixture(scope="module")
def slides64():
    """The eight D = 64 slides of COUNTS_64 with their own kmeans_fit results and the one-call ragged results (computed once)."""
    _lib.require_gpu()
    Xs = [getattr(synth, "features_" + kind)(40 + i, n, 64) for i, (kind, n) in enumerate(zip(KINDS_64, COUNTS_64))]
    return Xs, [alone(x) for x in Xs], ragged(Xs)


def test_seeding_classes_and_tile_edges_in_one_call(slides64):
    Xs, ref, r = slides64
    assert len(r["labels"]) == 8 and tuple(r["cluster_features"].shape) == (8, 100, 64) and tuple(r["indices"].shape) == (8, 100)
    assert r["labels"][0].dtype == torch.int32 and [int(l.numel()) for l in r["labels"]] == COUNTS_64
    for i in range(8):
        assert same(slide_of(r, i), ref[i]), (i, COUNTS_64[i])
    for i in range(8):                                       # every slide against the oracle: both sides of both class borders
        assert same(slide_of(r, i), oracle(Xs[i])), COUNTS_64[i]


def test_sliced_product_d512(gold):
    """D = 512 takes the eight-slice centre x point product: a slide's planes lie behind those of the slides before it."""
    Xs = [synth.features_gmm(8, 257, 512), synth.features_lowrank(50, 1000, 512), synth.features_normal(51, 130, 512),
          synth.features_gmm(52, 1100, 512)]
    r = ragged(Xs)
    assert np.array_equal(r["labels"][0].cpu().numpy(), gold["gmm_8_512_n257::labels"])
    for i, x in enumerate(Xs):
        assert same(slide_of(r, i), alone(x)), i
    assert same(slide_of(r, 3), oracle(Xs[3]))               # the planes behind three other slides' against the oracle


def test_golden_anchors_d1024(gold):
    Xs = [synth.features_gmm(0, 1000, 1024), synth.features_gmm(53, 300, 1024), synth.features_lowrank(54, 1500, 1024),
          synth.features_lowrank(2, 1000, 1024)]
    r = ragged(Xs)
    for i, tag in ((0, "gmm_0_1024"), (3, "lowrank_2_1024")):
        got = slide_of(r, i)
        assert np.array_equal(got[1], gold[tag + "::indices"]), "k-means++ seeding order"
        assert np.array_equal(got[0], gold[tag + "::labels"])
        assert got[2] == int(gold[tag + "::n_iter"])
        assert np.array_equal(got[3], gold[tag + "::cluster_features"])      # bitwise


def test_position_and_company(slides64):
    Xs, ref, _ = slides64
    rev = ragged(Xs[::-1])
    for i in range(8):
        assert same(slide_of(rev, i), ref[7 - i]), i
    one = ragged([Xs[2]])
    assert same(slide_of(one, 0), ref[2])
    Es = np.stack([synth.features_lowrank(20 + i, 600, 256) for i in range(8)])
    b = kmeans_fit_batch(torch.from_numpy(Es).cuda(), 100)
    e = ragged(list(Es))
    assert np.array_equal(torch.stack(e["labels"]).cpu().numpy(), b["labels"].cpu().numpy())
    for key in ("indices", "n_iter", "cluster_features"):
        assert np.array_equal(e[key].cpu().numpy(), b[key].cpu().numpy()), key
    for i in (0, 7):                                         # the uniform batch itself against the oracle
        assert same((b["labels"][i].cpu().numpy(), b["indices"][i].cpu().numpy(), int(b["n_iter"][i]),
                     b["cluster_features"][i].cpu().numpy()), oracle(Es[i])), i
    # the (X_cat, counts) form of the input
    pair = kmeans_fit_ragged((torch.from_numpy(np.concatenate(Xs[:3])).cuda(), COUNTS_64[:3]), 100)
    for i in range(3):
        assert same(slide_of(pair, i), ref[i]), i


def test_pipeline_cluster_takes_a_list(slides64):
    from sequoia_pub_amd.pipeline import SlidePipeline
    Xs, ref, _ = slides64
    cf, labels = SlidePipeline(None, None).cluster([torch.from_numpy(x).cuda() for x in Xs[:3]])
    for i in range(3):
        assert np.array_equal(cf[i].cpu().numpy(), ref[i][3]) and np.array_equal(labels[i].cpu().numpy(), ref[i][0]), i


def test_uneven_convergence_and_empty_clusters():
    """The duplicate-rows slide of test_gpu_kmeans.py (40 distinct rows, 180 samples: stops after 2 iterations, relocation,
    NaN rows of empty clusters) between two slides that run on for many more bursts."""
    rs = np.random.RandomState(0)
    base = rs.randn(40, 64).astype(np.float32)
    dup = np.concatenate([base] * 5)[:180]
    Xs = [synth.features_lowrank(31, 700, 64), dup, synth.features_lowrank(32, 700, 64)]
    ref = [alone(x) for x in Xs]
    r = ragged(Xs)
    got = [slide_of(r, i) for i in range(3)]
    print("n_iter", [g[2] for g in got])
    assert got[1][2] == 2 and np.isnan(got[1][3]).any() and got[0][2] > 6 and got[2][2] > 6
    assert not np.isnan(got[0][3]).any() and not np.isnan(got[2][3]).any()
    for i in range(3):
        assert same(got[i], ref[i], equal_nan=(i == 1)), i


def test_budget_split_and_large_slide(slides64):
    Xs, ref, r = slides64
    budget = 100 << 20
    assert len(ragged_plan(COUNTS_64, 64, 100, budget)) == 3
    cut = ragged(Xs, max_workspace_bytes=budget)
    for i in range(8):
        assert same(slide_of(cut, i), slide_of(r, i)), i
    big = synth.features_gmm(60, 4100, 64)                     # above GRAM_MAX_ROWS: the large-slide route, alone
    assert [g[2] for g in ragged_plan([600, 4100, 257], 64, 100, 4 << 30)] == ["gram", "large", "gram"]
    m = ragged([Xs[2], big, Xs[1]])
    assert same(slide_of(m, 1), alone(big))
    assert same(slide_of(m, 1), oracle(big))                 # the large route, anchored outside the code under test
    assert same(slide_of(m, 0), ref[2]) and same(slide_of(m, 2), ref[1])


def test_refusals():
    with pytest.raises(ValueError):
        ragged([synth.features_gmm(1, 300, 64), synth.features_gmm(2, 50, 64)])
    with pytest.raises(_lib.SequoiaHipError):
        kmeans_fit_ragged([torch.zeros(300, 64).cuda(), torch.zeros(300, 64)], 100)
    with pytest.raises(ValueError):
        kmeans_fit_ragged([torch.zeros(300, 64).cuda(), torch.zeros(300, 128).cuda()], 100)
    L = _lib.lib()
    ns = np.array([300, 4097], np.int32)
    fc = np.zeros(2, np.int32)
    rc = L.sq_kmeans_fit_ragged(None, 2, ns.ctypes.data, 64, 100, fc.ctypes.data, None, 1, 300, 1e-4, None, None, None, None, None, 0, None)
    assert rc != 0 and b"n_samples=4097" in L.sq_last_error()


def test_cli_batch_slides_writes_the_same_bytes(tmp_path, capsys):
    import pandas as pd
    from sequoia_pub_amd import store
    from sequoia_pub_amd.cli import kmean_features
    root = str(tmp_path)
    names = [f"TCGA-BB-{i:04d}" for i in range(6)]
    counts = [120, 60, 300, 450, 200, 1030]                   # 60: fewer patches than clusters; slide 4 is already clustered
    done = np.full((100, 64), 7.0, np.float32)
    for i, (name, n) in enumerate(zip(names, counts)):
        d = os.path.join(root, "a", "TCGA-BRCA", name)
        os.makedirs(d)
        f = store.File(os.path.join(d, name + ".h5"), "w")
        f.create_dataset("resnet_features", data=synth.features_gmm(70 + i, n, 64))
        if i == 4:
            f.create_dataset("cluster_features", data=done)
        f.close()
    shutil.copytree(os.path.join(root, "a"), os.path.join(root, "b"))
    shutil.copytree(os.path.join(root, "a"), os.path.join(root, "untouched"))
    ref = os.path.join(root, "ref.csv")
    pd.DataFrame([dict(wsi_file_name=n + ".svs", patient_id=n, tcga_project="TCGA-BRCA") for n in names]).to_csv(ref, index=False)
    out = {}
    for tree, batch in (("a", "1"), ("b", "4")):
        kmean_features.main(["--ref_file", ref, "--feature_path", os.path.join(root, tree), "--batch_slides", batch])
        out[tree] = capsys.readouterr().out
    assert out["a"] == out["b"] and "less number of patches" in out["a"] and "already available" in out["a"]
    for i, name in enumerate(names):
        a, b = (os.path.join(root, t, "TCGA-BRCA", name, name + ".h5") for t in ("a", "b"))
        with store.File(a, "r") as fa, store.File(b, "r") as fb:
            if i == 1:
                assert "cluster_features" not in fa.keys() and "cluster_features" not in fb.keys()
                continue
            ca, cb = np.asarray(fa["cluster_features"][:]), np.asarray(fb["cluster_features"][:])
            assert ca.shape == (100, 64) and ca.tobytes() == cb.tobytes(), name
            if i == 4:
                assert np.array_equal(ca, done)
        assert filecmp.cmp(a, b, shallow=False), name         # whole files byte-identical
        if i in (1, 4):                                       # the skipped ones are what they were
            assert filecmp.cmp(a, os.path.join(root, "untouched", "TCGA-BRCA", name, name + ".h5"), shallow=False), name
