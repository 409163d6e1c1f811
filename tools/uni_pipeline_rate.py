"""slides/s of SlidePipeline with the UNI ViT-L/16 embedder in one numeric mode, on slides resident in HBM.  bench.py's
pipeline workload routes only fp32 / bf16 to the UNI embedder; this is the same recipe (create_model, LayerScale gains 0.3,
1000 synthetic 224 px patches per slide, k-Means(100), ViS with bench.py's configuration, fp32 aggregator for the split mode)
for comparing the modes, f16x3 included, in one call:
    python tools/uni_pipeline_rate.py --dtype f16x3 --slides 2 --steps 3 --warmup 1 [--sub-batch 256]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import synth  # noqa: E402
from sequoia_pub_amd.pipeline import SlidePipeline  # noqa: E402
from sequoia_pub_amd.uni import create_model  # noqa: E402
from sequoia_pub_amd.vis import ViS  # noqa: E402

VIS_CFG = dict(num_outputs=20820, input_dim=1024, depth=6, nheads=16, dimensions_f=64, dimensions_s=64, dimensions_c=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16x3", choices=["fp32", "bf16", "f16x3"])
    ap.add_argument("--slides", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sub-batch", type=int, default=0, help="patches per launch group (default: 1000 in bf16, else 256, as bench.py)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(99)
    rn = create_model(compute_dtype=args.dtype).to(dev).eval()
    with torch.no_grad():
        for k, (off, shape) in rn._tmap.items():
            if k.endswith("gamma"):
                rn.flat[off:off + shape[0]] = 0.3
    vis = ViS(**VIS_CFG, num_clusters=100, device=str(dev), compute_dtype="fp32" if args.dtype == "f16x3" else args.dtype).to(dev).eval()
    sub = args.sub_batch or (1000 if args.dtype == "bf16" else 256)
    pipe = SlidePipeline(rn, vis, sub_batch=sub)
    slides = [torch.from_numpy(synth.patches_u8(i, 1000, 224)).to(dev) for i in range(args.slides)]
    for _ in range(args.warmup):
        pipe(slides)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = pipe(slides)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rate = args.steps * args.slides / dt
    print(json.dumps({"embedder": "uni", "dtype": args.dtype, "sub_batch": sub, "slides_per_step": args.slides, "steps": args.steps,
                      "seconds": round(dt, 3), "slides_per_s": round(rate, 3), "finite": bool(torch.isfinite(out["pred"]).all()),
                      "nonfinite_reruns": int(getattr(pipe, "nonfinite_reruns", 0))}))


if __name__ == "__main__":
    main()
