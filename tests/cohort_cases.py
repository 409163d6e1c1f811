"""Shapes and the tiny-cohort writer shared by tests/test_cohort_host.py (CPU) and tests/test_gpu_cohort.py (GPU): the
device-resident cohort feed (sequoia_pub_amd.data: CohortTable, ResidentLoader; csrc/cohort.hip: sq_cohort_gather)."""
import os

import numpy as np
import pandas as pd

from sequoia_pub_amd import store

# (S, tokens, D, G, index) of the gather against torch indexing; index None: the identity
GATHER_CASES = [
    (5, 3, 5, 7, [4, 0, 0, 2]),                        # nothing is 16-byte aligned (rows of 15 and 7 floats), an index repeats
    (6, 100, 32, 30, [5, 2, 0, 3, 1, 4]),              # x rows aligned, y rows (30 floats) not
    (5, 100, 1024, 20820, [3, 1, 4]),                  # the real widths, all rows aligned
    (5, 3, 5, 7, None),
    (6, 100, 32, 30, None),
]
GUARD_SHAPES = [(5, 3, 5, 7), (5, 100, 1024, 20820)]    # index [-1, 5, 2] at S = 5 on the dword and on the 16-byte path
OUT_OF_RANGE = [-1, 5, 2]

# the first table whose rows reach beyond 2^31 bytes: row 5243 is the first whose byte offset exceeds 2^31
BIG_S, BIG_TOKENS, BIG_D = 5300, 100, 1024
BIG_ROWS = [5299, 0, 5242]
assert 5242 * BIG_TOKENS * BIG_D * 4 <= 2 ** 31 < 5243 * BIG_TOKENS * BIG_D * 4     # row 5242 straddles 2^31, row 5299 lies beyond

MISSING, NO_DATASET, FLOAT64 = 2, 3, 5                 # the odd slides of the 7-slide cohort


def slide_name(i):
    return f"TCGA-AA-{i:04d}"


def write_cohort(root, extra=0, tokens=4, dim=8, genes=5, seed=0, odd=True, project="TCGA-BRCA"):
    """7 + ``extra`` slides under ``root``/features, one patient each; with ``odd`` slide 2 has no store file, slide 3 a store
    without ``cluster_features`` and slide 5 stores float64 (values that float32 cannot hold exactly).  Returns (frame, feature_path)."""
    rs = np.random.RandomState(seed)
    feature_path = os.path.join(str(root), "features")
    rows = []
    for i in range(7 + extra):
        name = slide_name(i)
        d = os.path.join(feature_path, project, name)
        os.makedirs(d)
        if not (odd and i == MISSING):
            with store.File(os.path.join(d, name + ".h5"), "w") as f:
                if odd and i == NO_DATASET:
                    f.create_dataset("resnet_features", data=rs.rand(9, dim).astype(np.float32))
                elif odd and i == FLOAT64:
                    f.create_dataset("cluster_features", data=rs.rand(tokens, dim) / 3.0)
                else:
                    f.create_dataset("cluster_features", data=rs.rand(tokens, dim).astype(np.float32))
        rows.append(dict(wsi_file_name=name, patient_id=f"P{i}", tcga_project=project,
                         **{f"rna_G{g}": float(rs.rand() * 6) for g in range(genes)}))
    return pd.DataFrame(rows), feature_path
