"""Writes tests/golden/emd.npz: the optimum of every case of tests/emd_cases.py from scipy.optimize.linprog(method="highs"),
the independent witness of the device's earth mover's distance.  A value is admitted only with linprog's OWN certificate
-- its flow and the marginals of its equality constraints pass emd_cases.check_certificate within the same bounds the
device is held to; a case whose linprog result misses them is given another seed in emd_cases.py, never a wider bound.

    python tests/golden/make_emd_golden.py

Needs scipy; runs on the host, no GPU."""
import os
import sys

import numpy as np
import scipy
import scipy.sparse as sp
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emd_cases as ec  # noqa: E402


def lp_emd(arr0, arr1, label):
    """calculate_emd's conventions around the linear program's optimum; the certificate is asserted before returning."""
    s0, s1 = ec.signature(arr0), ec.signature(arr1)
    if s0 is None and s1 is None:
        return 0.0
    if s0 is None or s1 is None:
        return float("nan")
    (ca, wa), (cb, wb) = s0, s1
    n, m = len(wa), len(wb)
    c = ec.cost_matrix(ca, cb)
    rows = sp.kron(sp.identity(n), np.ones((1, m)))           # x is the flow, row-major [n, m]
    cols = sp.kron(np.ones((1, n)), sp.identity(m))
    res = linprog(c.ravel(), A_eq=sp.vstack([rows, cols]).tocsr(), b_eq=np.concatenate([wa, wb]), bounds=(0, None), method="highs")
    assert res.status == 0, (label, res.message)
    flow = np.maximum(res.x.reshape(n, m), 0.0)
    ij = np.argwhere(flow > 0)
    dual = np.asarray(res.eqlin.marginals)
    ec.check_certificate(wa, wb, (ca, cb), dual[:n], dual[n:], (ij, flow[ij[:, 0], ij[:, 1]]), res.fun, label="linprog " + label)
    return float(res.fun)


def main():
    out = {}
    for name, case in ec.cases().items():
        out[name + "_value"] = np.array([lp_emd(*ec.grids_of(case), name)])
        out[name + "_crc"] = np.array([ec.case_crc(case)], dtype=np.int64)
    arr0, arr1 = ec.batch_case()
    out["batch_values"] = np.array([lp_emd(a, b, f"batch {p}") for p, (a, b) in enumerate(zip(arr0, arr1))])
    out["batch_crc"] = np.array([ec.crc(arr0, arr1)], dtype=np.int64)
    a, b, xtf, ytf = ec.table_case()
    out["table_values"] = np.array([lp_emd(*ec.fill_shift(a[:, ja], b[:, jb], xtf, ytf), f"table {p}")
                                    for p, (ja, jb) in enumerate(zip(ec.TABLE_COLS_A, ec.TABLE_COLS_B))])
    out["table_crc"] = np.array([ec.crc(a, b, xtf, ytf)], dtype=np.int64)
    # the pair at the cell limit has 4096 x 4096 variables, beyond linprog here: its value is the RESTATEMENT's, admitted with
    # the restatement's own certificate (which proves it), and named for what it is
    arr0, arr1 = ec.limit_case()
    (ca, wa), (cb, wb) = ec.signature(arr0), ec.signature(arr1)
    value, u, v, ij, f, stats = ec.solve(wa, ca, wb, cb)
    ec.check_certificate(wa, wb, (ca, cb), u, v, (ij, f), value, label=f"restatement limit ({stats})")
    out["limit_restated_value"] = np.array([value])
    out["limit_crc"] = np.array([ec.crc(arr0, arr1)], dtype=np.int64)
    np.savez(os.path.join(HERE, "emd.npz"), **out)
    print(f"scipy {scipy.__version__}: wrote {len(out)} arrays to {os.path.join(HERE, 'emd.npz')}")
    for k in sorted(out):
        if not k.endswith("_crc"):
            print(k, out[k])


if __name__ == "__main__":
    main()
