"""ms per slide of k-Means(100) + cluster means on slides around and above the Gram route's 4096-patch limit:
    python tools/kmeans_large_rate.py [--calls 10] [--warmup 2] [--no-cpu] [--out profiles/kmeans_large_rate.txt]
Slides (synth.features_gmm, seed 300 + i): 4096x2048 through BOTH routes, then 8192x2048, 20000x2048, 50000x1024 through
the large-slide route.  Per slide: warm-up, then `calls` timed calls ended by one device synchronise.  The split is taken
with a second timed loop at max_iter = 0 (centring + seeding + the one forced E-step + cluster means): "seeding" is that
time, "lloyd" the rest of the full call.  The CPU column is scikit-learn's KMeans(100, random_state=0).fit + the per-label
means on the host threads this process may use (one run; oracle.kmeans_oracle.kmeans_fit when scikit-learn cannot be
imported -- the line says which).  Prints one line per slide and a last JSON line; --out also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import synth  # noqa: E402
from sequoia_pub_amd.kmeans import GRAM_MAX_ROWS, kmeans_fit  # noqa: E402

SLIDES = [(4096, 2048, "gram"), (4096, 2048, "large"), (8192, 2048, "large"), (20000, 2048, "large"), (50000, 1024, "large")]


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, r


def cpu_fit(X):
    """(seconds, what ran, labels)"""
    try:
        from sklearn.cluster import KMeans
        t0 = time.perf_counter()
        km = KMeans(n_clusters=100, random_state=0).fit(X)
        np.asarray([np.mean(X[np.where(km.labels_ == pos)], axis=0) for pos in range(100)])
        return time.perf_counter() - t0, "scikit-learn", km.labels_
    except ImportError:
        from oracle import kmeans_oracle as ko
        t0 = time.perf_counter()
        r = ko.kmeans_fit(X)
        ko.cluster_means(X, r["labels"])
        return time.perf_counter() - t0, "oracle.kmeans_oracle", r["labels"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 1
    lines, rows, cpu_cache = [], [], {}
    for i, (n, dim, route) in enumerate(SLIDES):
        seed = 300 + (0 if n == GRAM_MAX_ROWS else i)
        Xh = synth.features_gmm(seed, n, dim)
        X = torch.from_numpy(Xh).cuda()
        full, r = timed(lambda: kmeans_fit(X, 100, route=route), args.calls, args.warmup)
        seeding, _ = timed(lambda: kmeans_fit(X, 100, max_iter=0, route=route), args.calls, 1)
        row = dict(n=n, dim=dim, route=route, ms=round(full, 3), seeding_ms=round(seeding, 3), lloyd_ms=round(full - seeding, 3),
                   n_iter=int(r["n_iter"][0]))
        if not args.no_cpu:
            if (seed, n, dim) not in cpu_cache:
                cpu_cache[(seed, n, dim)] = cpu_fit(Xh)
            sec, what, lab = cpu_cache[(seed, n, dim)]
            row.update(cpu_ms=round(sec * 1e3, 1), cpu=what, cpu_threads=torch.get_num_threads(), ratio=round(sec * 1e3 / full, 1),
                       labels_differing_from_cpu=int((r["labels"][0].cpu().numpy() != lab).sum()))
        rows.append(row)
        lines.append(f"{n:6d} x {dim:4d}  {route:5s}  {full:9.3f} ms  (seeding {seeding:8.3f}, lloyd {full - seeding:8.3f}, n_iter {row['n_iter']:3d})"
                     + ("" if args.no_cpu else f"  {row['cpu']} on {row['cpu_threads']} threads {row['cpu_ms']:9.1f} ms = {row['ratio']:.1f}x"
                        f"  labels differing {row['labels_differing_from_cpu']}"))
        print(lines[-1], flush=True)
        del X
    lines.append(json.dumps(dict(calls=args.calls, warmup=args.warmup, rows=rows)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
