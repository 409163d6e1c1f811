"""Makes tests/golden/gtalign.npz from the reference's LITERAL functions: spatial_vis/get_emd.py is imported as it stands
(cv2, ot and scanpy, which it imports and these functions never touch, are stubbed; matplotlib and tqdm too where absent) and
    get_average       is called once per tile -- with the spot index as the expression and the module's np.mean watched, the
                      literal sorted(...)[:num_tiles] gives the kept indices in order; with the real expression, the mean
    median_filter     is called once per row, on the frame after the literal dropna where NaN means absent
    score2percentile  row by row, and len(np.unique(...)), for the whole chain of :164-175 and :204-205
on the inputs tests/gtalign_cases.py defines (regenerated from their seeds by the tests; only a checksum of each is stored).
Run from the repository root:  python tests/golden/make_gtalign_golden.py --reference <the reference's spatial_vis folder>"""
import argparse
import importlib.util
import os
import sys
import types
import warnings
import zlib

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gtalign_cases as gc  # noqa: E402


def load_get_emd(folder):
    """Import <folder>/get_emd.py; its script part is behind ``if __name__ == '__main__'`` and does not run."""
    for name in ("cv2", "ot", "scanpy", "tqdm", "matplotlib", "matplotlib.pyplot", "matplotlib.cm"):
        try:
            if name in ("cv2", "ot", "scanpy"):
                raise ImportError
            __import__(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.rcParams, stub.tqdm = {}, (lambda it, *a, **k: it)
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("reference_get_emd", os.path.join(folder, "get_emd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.array([c], dtype=np.int64)


class WatchedNumpy:
    """The module's ``np`` with ``mean`` recording its argument: what get_average hands to np.mean is the kept values."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, values, *args, **kwargs):
        self.seen.append(list(values))
        return np.mean(values, *args, **kwargs)


def literal_indices(ref, xc, yc, sx, sy, k):
    df = pd.DataFrame({"x": sx, "y": sy})
    df["gene_expr"] = np.arange(len(sx), dtype=np.float64)
    watched, real = WatchedNumpy(), ref.np
    ref.np = watched
    try:
        for x, y in zip(xc, yc):
            ref.get_average(x, y, df, k)
    finally:
        ref.np = real
    return np.array(watched.seen, dtype=np.float64).astype(np.int32)


def literal_means(ref, xc, yc, sx, sy, column, k):
    df = pd.DataFrame({"x": sx, "y": sy})
    df["gene_expr"] = column                                   # an f32 column stays f32 in the frame
    return np.array([ref.get_average(x, y, df, k) for x, y in zip(xc, yc)], dtype=np.float64)


def literal_median(ref, values, xtf, ytf, r, nan_absent):
    out = np.full(values.shape, np.nan)
    for c in range(values.shape[1]):
        df = pd.DataFrame({"xcoord_tf": xtf, "ycoord_tf": ytf, "v": values[:, c]})
        if nan_absent:
            df = df.dropna(axis=0, how="any")
        res = df.apply(lambda row: ref.median_filter(df, "v", row["xcoord_tf"], row["ycoord_tf"], r), axis=1)
        out[df.index.values, c] = res.values
    return out


def literal_chain(ref, out):
    """get_emd.py:157-158, :163-175 and :204-205 for every requested gene, the frames built in memory."""
    w = gc.whole_case()
    for j, gene in enumerate(gc.WHOLE_GENES):
        df = pd.DataFrame({"x": w["spot_x"], "y": w["spot_y"]})
        df["gene_expr"] = w["spot_expr"][:, j]
        df2 = pd.DataFrame({"xcoord": w["xcoord"], "ycoord": w["ycoord"], "xcoord_tf": w["xtf"], "ycoord_tf": w["ytf"]})
        for name, col in zip(gc.WHOLE_NAMES, w["pred"].T):
            df2[name] = col.astype(np.float64)
        num_tiles = 4
        df2 = df2.dropna(axis=0, how="any")
        df2["ground_truth"] = df2.apply(lambda row: ref.get_average(row["xcoord"], row["ycoord"], df, num_tiles=num_tiles), axis=1)
        df2 = df2.dropna(axis=0, how="any")
        df2["ground_truth_filt"] = df2.apply(lambda row: ref.median_filter(df2, "ground_truth", row["xcoord_tf"], row["ycoord_tf"], 1), axis=1)
        refv = df2["ground_truth_filt"].values
        df2["ground_truth_filt"] = df2.apply(lambda row: ref.score2percentile(row["ground_truth_filt"], refv), axis=1)
        ref2 = df2[gene].values
        df2[gene + "_filt"] = df2.apply(lambda row: ref.score2percentile(row[gene], ref2), axis=1)
        out[f"whole_{gene}_rows"] = df2.index.values.astype(np.int64)
        out[f"whole_{gene}_ground_truth"] = df2["ground_truth"].values.astype(np.float64)
        out[f"whole_{gene}_ground_truth_filt"] = df2["ground_truth_filt"].values.astype(np.float64)
        out[f"whole_{gene}_filt"] = df2[gene + "_filt"].values.astype(np.float64)
        out[f"whole_{gene}_nr"] = np.array([len(np.unique(df2["ground_truth"].values)), len(np.unique(df2["ground_truth_filt"].values))],
                                           dtype=np.int64)
    out["whole_crc"] = crc(*gc.whole_case().values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the folder that holds the reference's get_emd.py (its spatial_vis)")
    args = ap.parse_args()
    ref = load_get_emd(args.reference)
    warnings.simplefilter("ignore", RuntimeWarning)                      # inf - inf and overflow are cases
    out = {}
    for name, (xc, yc, sx, sy, k) in gc.nearest_cases().items():
        out[f"ns_{name}_crc"] = crc(xc, yc, sx, sy)
        out[f"ns_{name}_idx"] = literal_indices(ref, xc, yc, sx, sy, k)
    for dtype in ("float32", "float64"):
        xc, yc, sx, sy, expr = gc.means_case(dtype)
        out[f"means_{dtype}_crc"] = crc(xc, yc, sx, sy, expr)
        for k in gc.MEANS_KS:
            out[f"means_{dtype}_k{k}"] = np.stack([literal_means(ref, xc, yc, sx, sy, expr[:, c], k) for c in gc.MEANS_COLS], axis=1)
    for name, (values, xtf, ytf) in gc.median_cases().items():
        out[f"mf_{name}_crc"] = crc(values, xtf, ytf)
        for r in gc.MEDIAN_RADII:
            for na in (0, 1):
                out[f"mf_{name}_r{r}_na{na}"] = literal_median(ref, values, xtf, ytf, r, na)
    for name, v in gc.unique_cases().items():
        out[f"uq_{name}_crc"] = crc(v)
        out[f"uq_{name}"] = np.array([len(np.unique(v))], dtype=np.int64)
    literal_chain(ref, out)
    np.savez_compressed(gc.GOLDEN, **out)
    print(gc.GOLDEN, os.path.getsize(gc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
