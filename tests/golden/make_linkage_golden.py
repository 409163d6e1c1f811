"""Writes tests/golden/linkage.npz: scipy's own pdist, linkage(..., method='average', metric='euclidean') and leaves_list on
the cases of tests/linkage_cases.py (inputs are rebuilt from their seeds there; only results are stored).
    python tests/golden/make_linkage_golden.py
Per case <name>_Z f64 [K-1, 4] and <name>_leaves int32 [K]; <name>_pdist (condensed f64) up to K = GOLDEN_DIST_MAX_K and
<name>_pdist_sha256 above; ``scipy_version``."""
import os
import sys

import numpy as np
import scipy
from scipy.cluster.hierarchy import dendrogram, leaves_list, linkage
from scipy.spatial.distance import pdist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import linkage_cases as lc  # noqa: E402


def main():
    out = {"scipy_version": np.array(scipy.__version__)}
    for name in lc.CASES:
        A = np.array(lc.case(name))
        d = pdist(A, "euclidean")
        Z = linkage(A, method="average", metric="euclidean")
        lv = leaves_list(Z).astype(np.int32)
        assert lv.tolist() == dendrogram(Z, no_plot=True)["leaves"]
        out[name + "_Z"], out[name + "_leaves"] = Z, lv
        if A.shape[0] <= lc.GOLDEN_DIST_MAX_K:
            out[name + "_pdist"] = d
        else:
            out[name + "_pdist_sha256"] = np.array(lc.digest(d))
    np.savez_compressed(lc.GOLDEN, **out)
    print(lc.GOLDEN, os.path.getsize(lc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
