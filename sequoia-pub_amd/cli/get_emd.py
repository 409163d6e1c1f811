"""Counterpart of the reference's spatial_vis/get_emd.py (whose paths are hard-coded): a predicted slide's
``stride-1.csv`` (what cli.visualize writes) is aligned with the slide's spatial-transcriptomics spots on the device
(gtalign.py) -- per gene the mean expression of every tile's four nearest spots, its 3 x 3 median over the tile grid, the
percentiles of both and of the prediction within the slide, and the number of distinct ground-truth values.

    python -m sequoia_pub_amd.cli.get_emd --slide_nr 242 --pred_folder gbm_celltypes --save_folder gbm_celltypes \\
        --gene_names EGFR,PDGFRA --ground_truth spots_242.csv

    python -m sequoia_pub_amd.cli.get_emd --slide_nr 242 --pred_folder gbm_celltypes --save_folder gbm_celltypes \\
        --gene_names EGFR,PDGFRA --h5ad auto

Keeps the reference's four flags (with its path conventions as defaults) and adds --pred_csv and --out as explicit paths
and the ground truth, exactly one of: --h5ad, the slide's raw anndata file, read and normalised on the device as the
reference does with scanpy (:148-155: normalize_total, log1p, scale -- spotnorm.py, once for all genes where the reference
redoes it per gene; f64, not scanpy's float32 digits), ``auto`` being the reference's path for --slide_nr; or
--ground_truth, a CSV with the columns ``x``, ``y`` and one ALREADY NORMALISED column per gene.  Writes
``<out>/metrics.csv`` (gene, nr_gt_vals, nr_gt_vals_filt) and ``<out>/aligned.csv``, the per-tile frame of
``gtalign.align_ground_truth``.  With --emd, metrics.csv is the reference's file: gene, emd, nr_gt_vals, emd_filt,
nr_gt_vals_filt -- the earth mover's distance between the predicted and the measured map, raw and as median-filtered
percentiles (emd.py: the optimum of the transportation problem in f64, where the reference calls cv2.EMD) -- and the
reference's line of ``slide_info.txt`` (:198-201: slide, grid rows squared, tiles of the first gene) is appended under
--out.  The figures stay out."""
import argparse
import os

import numpy as np
import pandas as pd
import torch

from .. import gtalign, spotnorm

H5AD_AUTO = os.path.join(".", "data", "Spatial_Heiland", "data", "AnnDataObject", "raw", "{nr}_T.h5ad")      # get_emd.py:148
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
    ap.add_argument("--ground_truth", default=None, help="CSV with the columns x, y and one already-normalised column per gene")
    ap.add_argument("--h5ad", default=None, help="the slide's raw .h5ad, normalised on the device (normalize_total, log1p, scale); "
                                                 "'auto': the reference's path for --slide_nr")
    ap.add_argument("--emd", action="store_true", help="also compute emd and emd_filt per gene and append the slide's line to slide_info.txt")
    ap.add_argument("--max_augmentations", type=int, default=None, help="with --emd: the cap on augmenting paths of one problem (default: 256 per cell of the two maps)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def parse_args(argv=None):
    """The parsed arguments with exactly one of --ground_truth and --h5ad, and ``--h5ad auto`` resolved."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if (args.ground_truth is None) == (args.h5ad is None):
        ap.error("exactly one of --ground_truth (a CSV of normalised spots) and --h5ad (the raw anndata file) must be given")
    if args.h5ad == "auto":
        if args.slide_nr is None:
            ap.error("--h5ad auto needs --slide_nr")
        args.h5ad = H5AD_AUTO.format(nr=args.slide_nr)
    return args


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


def write_slide_info(args, pred_csv, out, tiles, first_gene):
    """get_emd.py:198-201, once per slide: its name, arr0.shape[0] * arr1.shape[0] of the first gene's grid and that gene's
    number of tiles."""
    name = "HRI_" + str(args.slide_nr) + "_T.tif" if args.slide_nr is not None else os.path.basename(os.path.dirname(os.path.abspath(pred_csv)))
    present = tiles[~np.isnan(tiles[first_gene + "_ground_truth"].values)]
    height = int(present["xcoord_tf"].max()) + 1 if len(present) else 0
    with open(os.path.join(out, "slide_info.txt"), "a") as file:
        file.write(f"{name} \t {height * height} \t {len(present)} \n")


def main(argv=None):
    args = parse_args(argv)
    pred_csv, out = resolve_paths(args)
    genes = gene_list(args.gene_names)
    pred = pd.read_csv(pred_csv)
    truth = None if args.ground_truth is None else pd.read_csv(args.ground_truth)
    for frame, path, need in ((pred, pred_csv, COORDS + genes), (truth, args.ground_truth, ["x", "y"] + genes)):
        missing = [] if frame is None else [c for c in need if c not in frame.columns]
        if missing:
            raise SystemExit(f"{path} lacks the columns {missing[:8]}")
    names = [c for c in pred.columns if c not in COORDS and pd.api.types.is_numeric_dtype(pred[c])]
    device = torch.device(args.device)
    dev = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(device)      # noqa: E731
    if truth is None:
        spot_x, spot_y, spot_expr = spotnorm.spots_from_h5ad(args.h5ad, genes, device)
    else:
        spot_x, spot_y, spot_expr = dev(truth["x"].values, np.float64), dev(truth["y"].values, np.float64), dev(truth[genes].values, np.float64)
    tiles, metrics = gtalign.align_ground_truth(
        dev(pred[names].values, np.float32), names, dev(pred["xcoord"].values, np.float64), dev(pred["ycoord"].values, np.float64),
        dev(pred["xcoord_tf"].values, np.float64), dev(pred["ycoord_tf"].values, np.float64),
        spot_x, spot_y, spot_expr, genes, num_tiles=NUM_TILES,
        emd=args.emd, max_augmentations=args.max_augmentations)
    os.makedirs(out, exist_ok=True)
    if args.emd:
        write_slide_info(args, pred_csv, out, tiles, genes[0])
    metrics.to_csv(os.path.join(out, "metrics.csv"))
    tiles.to_csv(os.path.join(out, "aligned.csv"))
    print("Done")
    return metrics


if __name__ == "__main__":
    main()
