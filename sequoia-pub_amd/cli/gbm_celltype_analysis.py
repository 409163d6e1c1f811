"""Counterpart of /root/reference/spatial_vis/gbm_celltype_analysis.py (whose paths are hard-coded) without its figures:
per predicted slide ``<pred_folder>/<slide>/stride-1.csv`` (what cli.visualize writes) the gene-gene correlation of the
listed genes and the cell-type map -- category means, their percentiles within the slide, the colour of the leading
category -- computed on the device (mapstats.py), and the mean correlation over the slides.

    python -m sequoia_pub_amd.cli.gbm_celltype_analysis --pred_folder visualizations/spatial_GBM_pred/gbm_celltypes \\
        --all_genes gene_ids/gbm_experiments/all.npy --celltype_dir gene_ids/celltypes

Writes ``<pred_folder>/corr_maps/<slide>_corr.csv``, ``<pred_folder>/corr_maps/total_corr.csv`` and
``<pred_folder>/spatial_maps/<slide>.csv`` (xcoord_tf, ycoord_tf, per label its mean and percentile, color).

``--clustermap`` also writes what the reference's ``sns.clustermap`` figures (:81,145) are drawn from: per slide, and as
``total_*`` for the mean matrix, ``corr_maps/<slide>_clustered.csv`` (the correlation frame with rows and columns in the
leaf order of the average linkage of its rows), ``corr_maps/<slide>_linkage.csv`` (scipy's Z: left, right, distance, size)
and ``corr_maps/<slide>_order.csv`` (gene, color in leaf order: the row colours of the figure).  The mean matrix is
clustered over the genes present in every slide (its all-NaN rows and columns are dropped); a matrix that still holds a
NaN -- a constant gene -- is skipped with a printed line.

The gene list shrinks cumulatively over the slides as the reference's does (:70): slide k is correlated over the genes of
``all.npy`` present in slides 1..k; the maps (the reference's second loop, :91-111) use the genes present in every slide.
Where the reference's ``set`` leaves the order to chance, the order of ``all.npy`` is kept and slides are taken in sorted
order."""
import argparse
import os
from collections import OrderedDict

import numpy as np
import pandas as pd
import torch

from .. import mapstats

CELLTYPE_FILES = ("AC", "G1S", "G2M", "MES1", "MES2", "NPC1", "NPC2", "OPC")
# gbm_celltype_analysis.py:100-101
GROUPS = OrderedDict([("ac", ("AC",)), ("cc", ("G1S", "G2M")), ("mes", ("MES1", "MES2")), ("lin", ("NPC1", "NPC2", "OPC"))])
OUTPUT_FOLDERS = ("corr_maps", "spatial_maps")
COORDS = ["xcoord_tf", "ycoord_tf"]


def build_parser():
    ap = argparse.ArgumentParser(description="cell-type maps and gene co-expression of predicted slides")
    ap.add_argument("--pred_folder", required=True, help="holds <slide>/stride-1.csv; corr_maps/ and spatial_maps/ are written into it")
    ap.add_argument("--all_genes", required=True, help="all.npy: the genes to correlate")
    ap.add_argument("--celltype_dir", required=True, help="holds " + ", ".join(f + ".npy" for f in CELLTYPE_FILES))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--clustermap", action="store_true",
                    help="also write corr_maps/<slide>_clustered.csv, _linkage.csv and _order.csv (and total_*): the cluster maps' content")
    return ap


def group_categories(lists):
    """{'AC': [...], 'G1S': [...], ...} -> ordered {'ac': AC, 'cc': G1S + G2M, 'mes': MES1 + MES2, 'lin': NPC1 + NPC2 + OPC}."""
    return OrderedDict((label, [g for f in files for g in list(lists[f])]) for label, files in GROUPS.items())


def load_categories(celltype_dir):
    return group_categories({f: np.load(os.path.join(celltype_dir, f + ".npy"), allow_pickle=True).tolist() for f in CELLTYPE_FILES})


def gene_colors(categories, colors=None):
    """gene -> hex colour of its cell-type group: the reference's ``mapper`` (:42-56), a later group overriding an earlier one."""
    colors = mapstats.COLORS if colors is None else colors
    mapper = {}
    for label, genes in categories.items():
        mapper.update(dict.fromkeys(genes, colors[label]))
    return mapper


def write_clustermap(corr, name, folder, mapper, device):
    """The three files of one cluster map; returns False (and says why) where there is nothing to cluster."""
    if corr.shape[0] < 2:
        print(f"{name}: no cluster map -- the correlation matrix has {corr.shape[0]} genes, fewer than two")
        return False
    if bool(corr.isna().values.any()):
        print(f"{name}: no cluster map -- the correlation matrix holds a NaN (a constant gene)")
        return False
    order, clustered, Z = mapstats.cluster_order(corr, device=device, return_linkage=True)
    clustered.to_csv(os.path.join(folder, name + "_clustered.csv"))
    pd.DataFrame(Z.cpu().numpy(), columns=["left", "right", "distance", "size"]).to_csv(os.path.join(folder, name + "_linkage.csv"), index=False)
    genes = list(clustered.index)
    pd.DataFrame({"gene": genes, "color": [mapper.get(g, "") for g in genes]}).to_csv(os.path.join(folder, name + "_order.csv"), index=False)
    return True


def cumulative_genes(all_genes, slide_columns):
    """The gene list after each slide (:70, in the order of ``all_genes``): list k holds the genes present in slides 0..k."""
    genes, out = list(all_genes), []
    for columns in slide_columns:
        present = set(columns)
        genes = [g for g in genes if g in present]
        out.append(genes)
    return out


def slide_names(pred_folder):
    return sorted(d for d in os.listdir(pred_folder)
                  if d not in OUTPUT_FOLDERS and os.path.isfile(os.path.join(pred_folder, d, "stride-1.csv")))


def slide_frames(df, corr_genes, map_genes, categories, device):
    """One slide's frame (:64,72-75 and :95-111) -> (correlation frame over corr_genes, map frame over map_genes)."""
    df = df.dropna(axis=0, how="any")
    if not corr_genes:
        raise SystemExit("none of the listed genes is a column of the prediction table")
    table = torch.as_tensor(np.ascontiguousarray(df[corr_genes].values, dtype=np.float32)).to(device)
    corr = pd.DataFrame(mapstats.gene_correlation(table).cpu().numpy(), index=corr_genes, columns=corr_genes)
    if map_genes != corr_genes:
        where = {g: i for i, g in enumerate(corr_genes)}
        table = table[:, torch.as_tensor([where[g] for g in map_genes], dtype=torch.long, device=table.device)]
    maps = mapstats.celltype_maps(table, map_genes, categories, xtf=df["xcoord_tf"].values, ytf=df["ycoord_tf"].values)
    maps.index = df.index
    return corr, maps


def main(argv=None):
    args = build_parser().parse_args(argv)
    all_genes = np.load(args.all_genes, allow_pickle=True).tolist()
    categories = load_categories(args.celltype_dir)
    names = slide_names(args.pred_folder)
    if not names:
        raise SystemExit("no <slide>/stride-1.csv under " + args.pred_folder)
    for folder in OUTPUT_FOLDERS:
        os.makedirs(os.path.join(args.pred_folder, folder), exist_ok=True)
    paths = [os.path.join(args.pred_folder, name, "stride-1.csv") for name in names]
    gene_lists = cumulative_genes(all_genes, [pd.read_csv(p, nrows=0).columns for p in paths])
    corr_frames = []
    mapper = gene_colors(categories) if args.clustermap else None
    for name, path, genes in zip(names, paths, gene_lists):
        print(name)
        corr, maps = slide_frames(pd.read_csv(path), genes, gene_lists[-1], categories, args.device)
        corr.to_csv(os.path.join(args.pred_folder, "corr_maps", name + "_corr.csv"))
        maps.to_csv(os.path.join(args.pred_folder, "spatial_maps", name + ".csv"), index=False)
        corr_frames.append(corr)
        if args.clustermap:
            write_clustermap(corr, name, os.path.join(args.pred_folder, "corr_maps"), mapper, args.device)
    total = mapstats.mean_correlation(corr_frames)
    total.to_csv(os.path.join(args.pred_folder, "corr_maps", "total_corr.csv"))
    if args.clustermap:
        # the reference's sum_df carries NaN for every gene a later slide lacks (:70,137-140) and its clustermap call fails there
        shared = total.dropna(axis=0, how="all").dropna(axis=1, how="all")
        write_clustermap(shared, "total", os.path.join(args.pred_folder, "corr_maps"), mapper, args.device)
    return total


if __name__ == "__main__":
    main()
