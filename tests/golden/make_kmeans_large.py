"""scikit-learn golden results for slides of MORE than 4096 patches (the large-slide k-Means route).

Same recipe as ``gold_kmeans()`` in make_golden.py -- ``KMeans(100, random_state=0).fit(X)`` and ``_kmeans_plusplus``
on inputs from ``sequoia_pub_amd.synth`` -- for eleven seeded slides.  Per slide ``labels`` i32, ``indices`` i32 [100],
``n_iter`` and ``xsum`` (fp64 sum of X, pins the generator) go to tests/golden/kmeans_large.npz; no cluster means (the
tests take them from ``oracle.kmeans_oracle.cluster_means(X, labels)``, which the existing fixtures pin).

On large slides more points sit next to a cell border, so scikit-learn's fp32-sgemm Lloyd and the oracle's fp64 one can
part in a Lloyd step, not only at a seeding tie.  The script runs the oracle on every slide as well and sorts the slides:
label-equal ones are the golden cases (``cases`` in the .npz), the others go to kmeans_large_sklearn_mismatch.json with
the number of labels that differ.

    python tests/golden/make_kmeans_large.py          (needs scikit-learn; run in the build container)"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import synth  # noqa: E402
from oracle import kmeans_oracle as ko  # noqa: E402

SLIDES = [("gmm", 201, 4097, 64), ("lowrank", 202, 6000, 256), ("gmm", 203, 10000, 1024), ("gmm", 204, 20000, 256),
          ("normal", 205, 5000, 128), ("gmm", 206, 8192, 2048), ("lowrank", 207, 16384, 512), ("gmm", 208, 50000, 128),
          ("normal", 209, 12000, 64), ("gmm", 210, 4500, 2048), ("lowrank", 211, 30000, 64)]


def tag_of(kind, seed, n, dim):
    return f"{kind}_{seed}_{n}x{dim}"


def main():
    import sklearn
    from sklearn.cluster import KMeans
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    warnings.filterwarnings("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__)}
    equal, parted = [], []
    for kind, seed, n, dim in SLIDES:
        X = getattr(synth, "features_" + kind)(seed, n, dim)
        km = KMeans(n_clusters=100, random_state=0).fit(X)           # kmean_features.py:96
        Xc = X - X.mean(axis=0)
        _, idx = _kmeans_plusplus(Xc, 100, row_norms(Xc, squared=True), np.ones(len(X), np.float32), np.random.RandomState(0))
        tag = tag_of(kind, seed, n, dim)
        out[tag + "::labels"] = km.labels_.astype(np.int32)
        out[tag + "::indices"] = idx.astype(np.int32)
        out[tag + "::n_iter"] = np.array(km.n_iter_)
        out[tag + "::xsum"] = np.array(float(X.astype(np.float64).sum()))
        r = ko.kmeans_fit(X)
        differing = int((r["labels"] != km.labels_).sum())
        rec = dict(tag=tag, kind=kind, seed=seed, n=n, dim=dim, xsum=float(X.astype(np.float64).sum()),
                   indices_equal=bool(np.array_equal(idx, r["indices"])), labels_differing=differing,
                   n_iter_sklearn=int(km.n_iter_), n_iter_oracle=int(r["n_iter"]))
        (parted if differing or not rec["indices_equal"] or rec["n_iter_sklearn"] != rec["n_iter_oracle"] else equal).append(rec)
        print("kmeans_large", tag, "n_iter", km.n_iter_, "oracle n_iter", r["n_iter"], "labels differing", differing, flush=True)
    out["cases"] = np.array([r["tag"] for r in equal])
    out["mismatch_cases"] = np.array([r["tag"] for r in parted])
    np.savez_compressed(os.path.join(HERE, "kmeans_large.npz"), **out)
    json.dump(dict(sklearn_version=sklearn.__version__, numpy_version=np.__version__, scanned=[tag_of(*s) for s in SLIDES],
                   mismatches=parted,
                   note="oracle == scikit-learn on len(scanned) - len(mismatches) slides; on these the seeding is equal and the two part "
                        "in a Lloyd step (fp32 sgemm against fp64 distances for a point next to a cell border)"),
              open(os.path.join(HERE, "kmeans_large_sklearn_mismatch.json"), "w"), indent=1)
    print(len(SLIDES), "slides,", len(parted), "mismatches")


if __name__ == "__main__":
    main()
