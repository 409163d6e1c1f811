"""scikit-learn's results for the k-Means sweep of tests/kmeans_cases.py -> tests/golden/kmeans_sweep.npz.

Every case scikit-learn can express, by the call that expresses it:

    ROWS / STOP_CASES / BATCH_STOP   KMeans(k, random_state=0, max_iter=..., tol=...).fit(X): labels, n_iter; the seed indices
                                     from _kmeans_plusplus on the centred data with RandomState(0), as make_kmeans_large.py
    DBG_ROWS with sklearn=True       KMeans(k, init=C + mean, n_init=1, max_iter=..., tol=...).fit(X): labels, n_iter
    TRIAL_ROWS                       sklearn.cluster.kmeans_plusplus(Xc, k, n_local_trials=T): the seed indices.  Its draws come
                                     from a RandomState that replays the row's first centre and its table of uniforms.

Not expressible: max_iter = 0 (scikit-learn refuses it) and the exact-tie rows (DbgRow.sklearn False), where scikit-learn
orders equal distances by argpartition's internals.  `xsum` per case pins the generator.  Nothing of the oracle is stored:
tests/test_kmeans_cases_host.py compares the two.

    python tests/golden/make_kmeans_sweep.py          (needs scikit-learn; run in the build container)"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import kmeans_cases as kc  # noqa: E402
from oracle import kmeans_oracle as ko  # noqa: E402


class Replay(np.random.RandomState):
    """The draws of _kmeans_plusplus, given: choice() -> the first centre, uniform(size=T) -> the next row of the table."""

    def __init__(self, first, table):
        super().__init__(0)
        self._first, self._rows = first, iter(table)

    def choice(self, *a, **kw):
        return self._first

    def uniform(self, low=0.0, high=1.0, size=None):
        row = next(self._rows)
        assert size == len(row)
        return row.copy()


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    warnings.filterwarnings("ignore")
    out = {"sklearn_version": np.array(sklearn.__version__)}

    def put(tag, X, km=None, idx=None):
        out[tag + "::xsum"] = np.array(float(np.asarray(X, np.float64).sum()))
        if km is not None:
            out[tag + "::labels"] = km.labels_.astype(np.int32)
            out[tag + "::n_iter"] = np.array(km.n_iter_)
        if idx is not None:
            out[tag + "::indices"] = np.asarray(idx).astype(np.int32)
        print("kmeans_sweep", tag, "n_iter", None if km is None else km.n_iter_, flush=True)

    def seeds_of(X, k):
        Xc = X - X.mean(axis=0)
        return _kmeans_plusplus(Xc, k, row_norms(Xc, squared=True), np.ones(len(X), np.float32), np.random.RandomState(0))[1]

    for r in kc.ROWS:
        X = kc.row_data(r)
        put("row/" + r.name, X, KMeans(n_clusters=r.k, random_state=0).fit(X), seeds_of(X, r.k))
    stop = kc.ROW[kc.STOP_ROW]
    for c in kc.STOP_CASES:
        if c.max_iter >= 1:
            X = kc.row_data(stop)
            put("stop/" + c.name, X, KMeans(n_clusters=stop.k, random_state=0, max_iter=c.max_iter, tol=c.tol).fit(X))
    b = kc.BATCH_STOP
    for s, (kind, seed) in enumerate(zip(b.kinds, b.seeds)):
        X = kc.data(kind, seed, b.n, b.dim)
        put(f"batch/{s}", X, KMeans(n_clusters=b.k, random_state=0, max_iter=b.max_iter).fit(X), seeds_of(X, b.k))
    for r in kc.TRIAL_ROWS:
        X = kc.data(r.kind, r.seed, r.n, r.dim)
        Xc, _ = ko.center_data(X)
        _, idx = kmeans_plusplus(Xc, r.k, random_state=Replay(r.first, kc.trial_table(r.k, r.trials)), n_local_trials=r.trials)
        put("trial/" + r.name, X, None, idx)
    for r in kc.DBG_ROWS:
        if not r.sklearn:
            continue
        X, C = kc.dbg_inputs(r.name)
        for s in range(X.shape[0]):
            _, mean = ko.center_data(X[s])
            km = KMeans(n_clusters=C.shape[1], init=(C[s] + mean).astype(np.float32), n_init=1, max_iter=r.max_iter, tol=r.tol).fit(X[s])
            put(f"dbg/{r.name}/{s}", X[s], km)
    np.savez_compressed(os.path.join(HERE, "kmeans_sweep.npz"), **out)
    print(len(out) - 1, "arrays")


if __name__ == "__main__":
    main()
