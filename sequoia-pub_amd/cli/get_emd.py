"""Counterpart of the reference's spatial_vis/get_emd.py (whose paths are hard-coded) up to the EMD: a predicted slide's
``stride-1.csv`` (what cli.visualize writes) is aligned with the slide's spatial-transcriptomics spots on the device
(gtalign.py) -- per gene the mean expression of every tile's four nearest spots, its 3 x 3 median over the tile grid, the
percentiles of both and of the prediction within the slide, and the number of distinct ground-truth values.

    python -m sequoia_pub_amd.cli.get_emd --slide_nr 242 --pred_folder gbm_celltypes --save_folder gbm_celltypes \\
        --gene_names EGFR,PDGFRA --ground_truth spots_242.csv

Keeps the reference's four flags (with its path conventions as defaults) and adds --pred_csv and --out as explicit paths
and --ground_truth: a CSV with the columns ``x``, ``y`` and one ALREADY NORMALISED column per gene (the reference reads an
.h5ad and normalises it with scanpy: normalize_total, log1p, scale -- that stays with the caller).  Writes
``<out>/metrics.csv`` (gene, nr_gt_vals, nr_gt_vals_filt: the reference's file without its two emd columns) and
``<out>/aligned.csv``, the per-tile frame of ``gtalign.align_ground_truth``.  The EMD itself and the figures stay out
(DESIGN.md section 7)."""
import argparse
import os

import numpy as np
import pandas as pd
import torch

from .. import gtalign

COORDS = ["xcoord", "ycoord", "xcoord_tf", "ycoord_tf"]
NUM_TILES = 4             # get_emd.py:124: ground-truth spots per predicted tile


def build_parser():
    ap = argparse.ArgumentParser(description="align a predicted slide with its spatial-transcriptomics ground truth")
    ap.add_argument("--slide_nr", type=str, default=None, help="slide nr for which to run script")
    ap.add_argument("--pred_folder", type=str, default=None, help="folder with predictions to visualize")
    ap.add_argument("--save_folder", type=str, default=None, help="where to save results")
    ap.add_argument("--gene_names", type=str, required=True, help="names of genes (separated by comma) or path to npy array containing gene names")
    ap.add_argument("--pred_csv", default=None, help="the slide's stride-1.csv (default: from --slide_nr and --pred_folder, as the reference)")
    ap.add_argument("--out", default=None, help="output folder (default: from --slide_nr and --save_folder, as the reference)")
    ap.add_argument("--ground_truth", required=True, help="CSV with the columns x, y and one already-normalised column per gene")
    ap.add_argument("--device", default="cuda:0")
    return ap


def resolve_paths(args):
    """get_emd.py:106-122: the reference's folder conventions where no explicit path is given."""
    slide_name = None if args.slide_nr is None else "HRI_" + str(args.slide_nr) + "_T.tif"
    pred_csv, out = args.pred_csv, args.out
    if pred_csv is None:
        if slide_name is None or args.pred_folder is None:
            raise SystemExit("give --pred_csv, or --slide_nr and --pred_folder")
        pred_csv = os.path.join(".", "visualizations", "spatial_GBM_pred", args.pred_folder, slide_name, "stride-1.csv")
    if out is None:
        if slide_name is None or args.save_folder is None:
            raise SystemExit("give --out, or --slide_nr and --save_folder")
        out = os.path.join(".", "visualizations", "comparisons", args.save_folder, slide_name)
    return pred_csv, out


def gene_list(gene_names):
    if ".npy" in gene_names:
        return [str(g) for g in np.load(gene_names, allow_pickle=True).tolist()]
    return gene_names.split(",")


def main(argv=None):
    args = build_parser().parse_args(argv)
    pred_csv, out = resolve_paths(args)
    genes = gene_list(args.gene_names)
    pred = pd.read_csv(pred_csv)
    truth = pd.read_csv(args.ground_truth)
    for frame, path, need in ((pred, pred_csv, COORDS + genes), (truth, args.ground_truth, ["x", "y"] + genes)):
        missing = [c for c in need if c not in frame.columns]
        if missing:
            raise SystemExit(f"{path} lacks the columns {missing[:8]}")
    names = [c for c in pred.columns if c not in COORDS and pd.api.types.is_numeric_dtype(pred[c])]
    device = torch.device(args.device)
    dev = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(device)      # noqa: E731
    tiles, metrics = gtalign.align_ground_truth(
        dev(pred[names].values, np.float32), names, dev(pred["xcoord"].values, np.float64), dev(pred["ycoord"].values, np.float64),
        dev(pred["xcoord_tf"].values, np.float64), dev(pred["ycoord_tf"].values, np.float64),
        dev(truth["x"].values, np.float64), dev(truth["y"].values, np.float64), dev(truth[genes].values, np.float64), genes, num_tiles=NUM_TILES)
    os.makedirs(out, exist_ok=True)
    metrics.to_csv(os.path.join(out, "metrics.csv"))
    tiles.to_csv(os.path.join(out, "aligned.csv"))
    print("Done")
    return metrics


if __name__ == "__main__":
    main()
