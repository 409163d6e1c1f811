"""One slide's sliding-window map (spatial_vis/visualize.py:35-102, stride 1, feature cache resident in HBM) for the comparator
aggregators -- ViT (bf16, --model_type vit at the UNI width: dim 1024, depth 6, 16 heads, mlp 2048) and HE2RNA (fp32, layers
[256, 256], ks [1 .. 100]), G = 20 820 -- on the gather / vote path (spatial.sliding_window_method with three genes, as the CLI
asks; and the all-gene tensor form sliding_window_all_genes) and on the literal per-window form sliding_window_any_model, on a
100 x 100 grid; then the new path alone on BASELINE config 5's 250 x 200 grid.
    python tools/spatial_comparator_rate.py [--reps 2] [--skip-old] [--models vit_bf16,he2rna_fp32] [--grids 100x100,250x200]
Prints one JSON line (seconds per slide, the best of --reps after one warm-up)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd.he2rna import HE2RNA  # noqa: E402
from sequoia_pub_amd.spatial import sliding_window_all_genes, sliding_window_any_model, sliding_window_method  # noqa: E402
from sequoia_pub_amd.vit import ViT  # noqa: E402

G, D, GENES = 20820, 1024, [3, 17, 20819]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return round(best, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-old", action="store_true", help="leave out sliding_window_any_model")
    ap.add_argument("--models", default="vit_bf16,he2rna_fp32")
    ap.add_argument("--grids", default="100x100,250x200")
    args = ap.parse_args()
    names = args.models.split(",")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    models = {}
    if "vit_bf16" in names:
        models["vit_bf16"] = ViT(num_outputs=G, dim=D, depth=6, heads=16, mlp_dim=2048, device=str(dev), compute_dtype="bf16").to(dev).eval()
    if "he2rna_fp32" in names:
        models["he2rna_fp32"] = HE2RNA(input_dim=D, output_dim=G, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], device=str(dev)).eval()
    res = {"G": G, "D": D, "stride": 1}
    for nx, ny in (tuple(int(v) for v in g.split("x")) for g in args.grids.split(",")):
        xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        df = pd.DataFrame({"xcoord_tf": xs.ravel(), "ycoord_tf": ys.ravel()})
        feats = torch.relu(torch.randn(nx * ny, D, generator=torch.Generator().manual_seed(1))).to(dev)
        grid = f"{nx}x{ny}"
        for name, m in models.items():
            r = {"all_genes_s": timed(lambda: sliding_window_all_genes(df["xcoord_tf"].values, df["ycoord_tf"].values, feats, m, 1), args.reps)}
            if nx * ny <= 10000:
                r["method_3_genes_s"] = timed(lambda: sliding_window_method(df, feats, m, GENES, 1), args.reps)
                if not args.skip_old:
                    r["any_model_3_genes_s"] = timed(lambda: sliding_window_any_model(df, feats, m, GENES, 1, name.split("_")[0]), 1)
                    r["speedup"] = round(r["any_model_3_genes_s"] / r["method_3_genes_s"], 2)
            res[f"{name}_{grid}"] = r
            print(f"{name} {grid}: {r}", file=sys.stderr, flush=True)
        del feats
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
