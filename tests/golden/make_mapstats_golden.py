"""Makes tests/golden/mapstats.npz from the reference's LITERAL calls (spatial_vis/gbm_celltype_analysis.py):
    percentiles   df.apply(lambda row: score2percentile(row[label], ref), axis=1) -- one scipy.stats.percentileofscore per row
    means         df[[genes of the category]].mean(axis=1)
    label         df[[... '_perc']].idxmax(axis=1), '_perc' stripped, mapped to the colour
    correlation   df[genes].corr()
on the inputs tests/mapstats_cases.py defines (the inputs themselves are regenerated from their seeds by the tests; only a
checksum of each is stored).  Run from the repository root:  python tests/golden/make_mapstats_golden.py"""
import os
import sys
import zlib

import numpy as np
import pandas as pd
from scipy.stats import percentileofscore

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mapstats_cases as mc  # noqa: E402


def score2percentile(score, ref):                       # gbm_celltype_analysis.py:12-16
    if np.isnan(score):
        return score
    percentile = percentileofscore(ref, score)
    return percentile


def crc(a):
    return np.array([zlib.crc32(np.ascontiguousarray(a).tobytes())], dtype=np.int64)


def literal_percentiles(x):
    df = pd.DataFrame({f"c{k}": x[:, k] for k in range(x.shape[1])})
    out = {}
    for label in list(df.columns):
        ref = df[label].values
        out[label] = df.apply(lambda row: score2percentile(row[label], ref), axis=1)
    return np.stack([out[f"c{k}"].values for k in range(x.shape[1])], axis=1).astype(np.float64)


def literal_celltype_frame(x, names, categories_by_label, colors):
    """gbm_celltype_analysis.py:97-111 on a frame whose gene columns are f32 predictions read as f64 (the CSV's)."""
    df = pd.DataFrame(x.astype(np.float64), columns=names)
    df = df.dropna(axis=0, how="any")
    labels = list(categories_by_label.keys())
    categories = [categories_by_label[label] for label in labels]
    for j, label in enumerate(labels):
        df[label] = df[[i for i in categories[j] if i in df.columns]].mean(axis=1)
        ref = df[label].values
        df[label + "_perc"] = df.apply(lambda row: score2percentile(row[label], ref), axis=1)
    df["color"] = df[[i + "_perc" for i in labels]].idxmax(axis=1)
    df["color"] = df["color"].str.replace("_perc", "")
    label_of_row = df["color"].values.copy()
    df["color"] = df["color"].map(colors)
    return df, labels, label_of_row


def main():
    out = {}
    for name in mc.GOLDEN_PERC:
        x = mc.golden_percentile_input(name)
        out[name + "_crc"] = crc(x)
        out[name + "_out"] = literal_percentiles(x)
    x, names = mc.dyadic_table()
    df, labels, label_of_row = literal_celltype_frame(x, names, mc.dyadic_categories(), mc.COLORS)
    out["dyadic_crc"] = crc(x)
    out["dyadic_rows"] = df.index.values.astype(np.int64)
    out["dyadic_means"] = df[labels].values.astype(np.float64)
    out["dyadic_perc"] = df[[label + "_perc" for label in labels]].values.astype(np.float64)
    out["dyadic_label"] = np.array([labels.index(v) for v in label_of_row], dtype=np.int32)
    out["dyadic_color"] = np.array(df["color"].values.tolist())
    x = mc.nondyadic_table()
    frame = pd.DataFrame(x.astype(np.float64))
    out["nondyadic_crc"] = crc(x)
    out["nondyadic_means"] = np.stack([frame[cols].mean(axis=1).values for cols in mc.nondyadic_lists()], axis=1).astype(np.float64)
    for n, K in mc.CORR_SHAPES:
        x = mc.corr_input(n, K)
        out[f"corr_{n}_{K}_crc"] = crc(x)
        out[f"corr_{n}_{K}"] = pd.DataFrame(x.astype(np.float64)).corr().values.astype(np.float64)
    np.savez_compressed(mc.GOLDEN, **out)
    print(mc.GOLDEN, os.path.getsize(mc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
