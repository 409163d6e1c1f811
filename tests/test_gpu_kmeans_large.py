"""HIP k-Means on slides of more than 4096 patches (sq_kmeans_fit_large behind kmeans.kmeans_fit) against scikit-learn
golden labels (tests/golden/kmeans_large.npz), the CPU oracle and the Gram route.
Bar: labels, seeding indices and iteration counts equal; cluster means bit-equal (same fp32 add order).

Run alone:  timeout -k 10 600 python -m pytest -q -m gpu tests/test_gpu_kmeans_large.py"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import kmeans_oracle as ko  # noqa: E402  (checker only)
from sequoia_pub_amd import _lib, synth  # noqa: E402
from sequoia_pub_amd import kmeans as km_mod  # noqa: E402
from sequoia_pub_amd.kmeans import KMeans, kmeans_fit, kmeans_fit_batch  # noqa: E402

GOLDEN = [("gmm", 201, 4097, 64), ("lowrank", 202, 6000, 256), ("gmm", 203, 10000, 1024), ("normal", 205, 5000, 128),
          ("gmm", 206, 8192, 2048), ("lowrank", 207, 16384, 512), ("normal", 209, 12000, 64), ("gmm", 210, 4500, 2048),
          ("lowrank", 211, 30000, 64)]
SMALL_CASES = [("gmm", 0, 1024), ("gmm", 1, 2048), ("lowrank", 2, 1024), ("lowrank", 3, 2048),
               ("normal", 4, 1024), ("lowrank", 5, 256), ("gmm", 6, 1024)]          # CASES of tests/test_gpu_kmeans.py


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kmeans_large.npz"))


def _np(r):
    return {k: v[0].cpu().numpy() for k, v in r.items()}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("labels", "indices", "n_iter")) and \
        a["cluster_features"].tobytes() == b["cluster_features"].tobytes()


@pytest.mark.parametrize("kind,seed,n,dim", GOLDEN)
def test_large_slides_bit_equal_to_sklearn_golden(gold, kind, seed, n, dim):
    _lib.require_gpu()
    X = getattr(synth, "features_" + kind)(seed, n, dim)
    tag = f"{kind}_{seed}_{n}x{dim}"
    assert tag in [str(c) for c in gold["cases"]]
    km = KMeans(n_clusters=100, random_state=0).fit(X)          # kmean_features.py:96 on a slide of more than 4096 patches
    assert np.array_equal(km.seed_indices_, gold[tag + "::indices"]), "k-means++ seeding order"
    assert np.array_equal(km.labels_, gold[tag + "::labels"]), int((km.labels_ != gold[tag + "::labels"]).sum())
    assert km.n_iter_ == int(gold[tag + "::n_iter"])
    assert np.array_equal(km.cluster_features_, ko.cluster_means(X, gold[tag + "::labels"]))      # bitwise


def test_slides_where_oracle_and_sklearn_part_follow_the_oracle(gold, golden_dir):
    """The slides of kmeans_large_sklearn_mismatch.json (same seeding, a handful of border points assigned differently by
    scikit-learn's fp32 sgemm Lloyd): the HIP path implements the oracle's definition, so it gives the ORACLE's result,
    and the number of labels that differ from scikit-learn's is the recorded one."""
    _lib.require_gpu()
    fx = json.load(open(os.path.join(golden_dir, "kmeans_large_sklearn_mismatch.json")))
    assert len(fx["mismatches"]) >= 1
    for m in fx["mismatches"]:
        X = getattr(synth, "features_" + m["kind"])(m["seed"], m["n"], m["dim"])
        assert float(X.astype(np.float64).sum()) == m["xsum"]
        km = KMeans(n_clusters=100, random_state=0).fit(X)
        o = ko.kmeans_fit(X)
        assert np.array_equal(km.seed_indices_, o["indices"]), m["tag"]
        assert np.array_equal(km.labels_, o["labels"]), (m["tag"], int((km.labels_ != o["labels"]).sum()))
        assert km.n_iter_ == o["n_iter"]
        assert int((km.labels_ != gold[m["tag"] + "::labels"]).sum()) == m["labels_differing"]


@pytest.mark.parametrize("kind,seed,dim", SMALL_CASES)
def test_large_route_on_small_golden_slides(golden_dir, kind, seed, dim):
    """Both routes exist at n = 1000: the large one must give the scikit-learn golden results the Gram route gives."""
    _lib.require_gpu()
    g = np.load(os.path.join(golden_dir, "kmeans.npz"))
    X = getattr(synth, "features_" + kind)(seed, 1000, dim)
    r = _np(kmeans_fit(torch.from_numpy(X).cuda(), 100, route="large"))
    tag = f"{kind}_{seed}_{dim}"
    assert np.array_equal(r["indices"], g[tag + "::indices"])
    assert np.array_equal(r["labels"], g[tag + "::labels"])
    assert int(r["n_iter"]) == int(g[tag + "::n_iter"])
    assert np.array_equal(r["cluster_features"], g[tag + "::cluster_features"])      # bitwise


def test_large_route_equals_gram_route_at_4096():
    _lib.require_gpu()
    X = torch.from_numpy(synth.features_gmm(77, 4096, 2048)).cuda()
    a = _np(kmeans_fit_batch(X[None], 100))
    b = _np(kmeans_fit(X, 100, route="large"))
    assert np.array_equal(a["indices"], b["indices"]) and np.array_equal(a["labels"], b["labels"])
    assert int(a["n_iter"]) == int(b["n_iter"])
    assert a["cluster_features"].tobytes() == b["cluster_features"].tobytes()


def test_large_route_on_the_smallest_and_a_ragged_slide(golden_dir):
    """n = n_clusters (one tile, one chunk, every point its own cluster) and n = 257 (partial tile): as the Gram route."""
    _lib.require_gpu()
    for X in (synth.features_gmm(78, 100, 64), synth.features_gmm(8, 257, 512)):
        Xd = torch.from_numpy(X).cuda()
        assert _same(_np(kmeans_fit_batch(Xd[None], 100)), _np(kmeans_fit(Xd, 100, route="large")))
    r = _np(kmeans_fit(torch.from_numpy(synth.features_gmm(78, 100, 64)).cuda(), 100, route="large"))
    assert sorted(r["labels"].tolist()) == list(range(100))
    g = np.load(os.path.join(golden_dir, "kmeans.npz"))
    r = _np(kmeans_fit(torch.from_numpy(synth.features_gmm(8, 257, 512)).cuda(), 100, route="large"))
    assert np.array_equal(r["labels"], g["gmm_8_512_n257::labels"])


def _duplicates(rows):
    rs = np.random.RandomState(0)
    base = rs.randn(40, 64).astype(np.float32)
    return np.concatenate([base] * (rows // 40 + 1))[:rows]


def test_duplicate_points_and_empty_clusters_at_5000_rows():
    """test_duplicate_points_and_empty_clusters of tests/test_gpu_kmeans.py scaled to 5000 rows from 40 distinct ones
    (k = 100): exact ties, empty-cluster relocation and the stable member sort at n > 4096.  Once every distinct row is a
    centre every remaining distance is exactly 0 (norms and products share one association), the labels repeat in the
    second iteration: n_iter = 2, as the Gram route gives for the same construction cut to 4000 rows."""
    _lib.require_gpu()
    X = _duplicates(5000)
    km = KMeans(n_clusters=100, random_state=0).fit(X)
    small = KMeans(n_clusters=100, random_state=0).fit(_duplicates(4000))
    seeds = km.seed_indices_
    assert len({X[i].tobytes() for i in seeds}) == 40
    assert small.n_iter_ == 2 and km.n_iter_ == small.n_iter_
    first_dup = {}
    for c in range(100):
        first_dup.setdefault(X[seeds[c]].tobytes(), c)
    for j in range(len(X)):
        lab = km.labels_[j]
        assert np.array_equal(X[seeds[lab]], X[j])                     # assigned to a centre equal to the point
        assert lab == first_dup[X[j].tobytes()]                        # exact tie -> first index
    used = np.unique(km.labels_)
    assert len(used) == 40
    empty = np.setdiff1d(np.arange(100), used)
    assert len(empty) == 60
    assert np.isnan(km.cluster_features_[empty]).all() and not np.isnan(km.cluster_features_[used]).any()


def test_repeatable_and_independent_of_stale_workspace():
    """Two calls give the same bits; so does a raw call on a non-default stream over a workspace filled with 0xff."""
    _lib.require_gpu()
    Xh = synth.features_lowrank(202, 6000, 256)
    X = torch.from_numpy(Xh).cuda()
    a = _np(kmeans_fit(X, 100))
    b = _np(kmeans_fit(X, 100))
    assert _same(a, b)
    n, D, k = 6000, 256, 100
    L = _lib.lib()
    first, u = km_mod.seeding_draws(n, k, 0)
    u_dev = torch.from_numpy(u).cuda()
    need = L.sq_kmeans_large_workspace_bytes(n, D, k)
    assert need > 0
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ws = torch.full((need,), 0xff, dtype=torch.uint8, device="cuda")
        labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        means = torch.full((k, D), float("nan"), device="cuda")
        seeds = torch.full((k,), -7, dtype=torch.int32, device="cuda")
        n_iter = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        _lib.check(L.sq_kmeans_fit_large(_lib.ptr(X), n, D, k, first, _lib.ptr(u_dev), u.shape[1], 300, 1e-4, _lib.ptr(labels),
                                         _lib.ptr(means), _lib.ptr(seeds), _lib.ptr(n_iter), _lib.ptr(ws), need,
                                         ctypes.c_void_p(side.cuda_stream)))
    side.synchronize()
    c = dict(labels=labels.cpu().numpy(), indices=seeds.cpu().numpy(), n_iter=n_iter[0].cpu().numpy(), cluster_features=means.cpu().numpy())
    assert _same(a, c)


def test_bounds():
    _lib.require_gpu()
    bound = km_mod.LARGE_MAX_ROWS
    assert bound >= 65536
    L = _lib.lib()
    assert L.sq_kmeans_large_workspace_bytes(bound + 1, 64, 100) == 0
    # refused from the shape alone: a tensor that owns no memory of that size is enough, nothing is allocated or launched
    X = torch.zeros(1, 64, device="cuda").expand(bound + 1, 64)
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.SequoiaHipError, match=str(bound)):
        kmeans_fit(X, 100)
    assert torch.cuda.memory_allocated() == before
    # a workspace one byte short
    n, D, k = 5000, 64, 100
    Xs = torch.from_numpy(synth.features_normal(1, n, D)).cuda()
    first, u = km_mod.seeding_draws(n, k, 0)
    u_dev = torch.from_numpy(u).cuda()
    need = L.sq_kmeans_large_workspace_bytes(n, D, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    rc = L.sq_kmeans_fit_large(_lib.ptr(Xs), n, D, k, first, _lib.ptr(u_dev), u.shape[1], 300, 1e-4, _lib.ptr(labels), None, None, None,
                               _lib.ptr(ws), need - 1, _lib.stream_ptr(Xs.device))
    assert rc == -3 and b"workspace" in L.sq_last_error()          # SQ_ERR_WORKSPACE
    with pytest.raises(_lib.SequoiaHipError):
        kmeans_fit(torch.zeros(5000, 66, device="cuda"), 100)       # dim % 4


def test_cli_and_pipeline_take_a_5000_patch_slide(tmp_path, gold):
    """cli/kmean_features.py on a feature file with 5000 x 128 features, and SlidePipeline.cluster on the same tensor."""
    import pandas as pd
    from sequoia_pub_amd import store
    from sequoia_pub_amd.cli import kmean_features
    from sequoia_pub_amd.pipeline import SlidePipeline
    _lib.require_gpu()
    X = synth.features_normal(205, 5000, 128)
    lab = gold["normal_205_5000x128::labels"]
    want = ko.cluster_means(X, lab)
    slide = "TCGA-AA-0001"
    d = tmp_path / "features" / "TCGA-BRCA" / slide
    d.mkdir(parents=True)
    f = store.File(str(d / (slide + ".h5")), "w")
    f.create_dataset("resnet_features", data=X)
    f.close()
    ref = str(tmp_path / "ref.csv")
    pd.DataFrame([dict(wsi_file_name=slide + ".svs", patient_id="P0", tcga_project="TCGA-BRCA")]).to_csv(ref, index=False)
    kmean_features.main(["--ref_file", ref, "--feature_path", str(tmp_path / "features"), "--num_clusters", "100"])
    f = store.File(str(d / (slide + ".h5")), "r")
    got = np.asarray(f["cluster_features"][:])
    f.close()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    pipe = SlidePipeline(None, None, n_clusters=100)
    cf, labels = pipe.cluster(torch.from_numpy(X).cuda()[None])
    assert labels.shape == (1, 5000) and np.array_equal(labels[0].cpu().numpy(), lab)
    assert cf.shape == (1, 100, 128) and cf[0].cpu().numpy().tobytes() == want.tobytes()
