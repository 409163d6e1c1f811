"""ms per slide of k-Means(100) + cluster means over slides of DIFFERENT patch counts, one call per slide against one
ragged call (kmeans_fit_ragged), all in ONE run on one GPU:
    python tools/kmeans_ragged_rate.py [--rounds 5] [--calls 2] [--warmup 1] [--out profiles/kmeans_ragged_rate.txt]
(a) mixed cohort: 64 slides, patch counts RandomState(7).randint(300, 4001), D = 2048 (synth.features_gmm, seed 400 + i):
    kmeans_fit slide by slide -- the path every caller had before the ragged call, the yardstick of the same run -- against
    kmeans_fit_ragged on the list (which concatenates it) and on the (X_cat, counts) pair;
(b) equal counts, 8 x 1000 x 2048: kmeans_fit_batch against kmeans_fit_ragged -- what the table indirection costs where the
    uniform batch exists;
(c) the rows of (a) cut differently, same patch total: one 4000-patch slide among 63 equal ones against 64 equal ones --
    what grids sized by the largest slide cost.
The variants of a section alternate inside every round; a round times `calls` calls of each, ended by one device
synchronise.  Printed per variant: the median over the rounds and their min..max, in ms per slide; ratios are of medians.
(a) also checks that the ragged results equal the slide-by-slide ones.  --out also writes the lines to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, synth  # noqa: E402
from sequoia_pub_amd.kmeans import kmeans_fit, kmeans_fit_batch, kmeans_fit_ragged, ragged_plan  # noqa: E402

DIM = 2048


def mixed_counts(n_slides=64, lo=300, hi=4000, seed=7):
    return [int(c) for c in np.random.RandomState(seed).randint(lo, hi + 1, n_slides)]


def skewed_counts(total, n_slides=64, big=4000):
    """One `big` slide in the middle of n_slides - 1 equal ones, and n_slides equal ones; both sum to `total`."""
    def even(t, m):
        return [t // m + (1 if i < t % m else 0) for i in range(m)]
    rest = even(total - big, n_slides - 1)
    return rest[:n_slides // 2] + [big] + rest[n_slides // 2:], even(total, n_slides)


def alternate(variants, n_slides, rounds, calls, warmup):
    """variants: {name: fn}.  Returns {name: dict(median, min, max)} in ms per slide."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            got[name].append((time.perf_counter() - t0) / calls * 1e3 / n_slides)
    return {name: dict(median=float(np.median(v)), min=min(v), max=max(v)) for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slides", type=int, default=64, help="slides of the mixed cohort (smaller only to rehearse the script)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, report = [], dict(rounds=args.rounds, calls=args.calls, warmup=args.warmup, dim=DIM)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def table(title, res, base):
        say(title)
        for name, r in res.items():
            say(f"  {name:44s} {r['median']:8.4f} ms per slide  (rounds {r['min']:.4f} .. {r['max']:.4f})"
                + ("" if name == base else f"  = {r['median'] / res[base]['median']:.3f} x {base}"))

    # (a) the mixed cohort
    counts = mixed_counts(args.slides)
    S, total = len(counts), sum(counts)
    Xcat = torch.cat([torch.from_numpy(synth.features_gmm(400 + i, n, DIM)) for i, n in enumerate(counts)]).cuda()
    slides = list(Xcat.split(counts))
    plan = ragged_plan(counts, DIM, 100, 4 << 30)
    loop = [kmeans_fit(x, 100) for x in slides]
    rag = kmeans_fit_ragged((Xcat, counts), 100)
    for i in range(S):
        assert torch.equal(rag["labels"][i], loop[i]["labels"][0]) and torch.equal(rag["indices"][i], loop[i]["indices"][0]), i
        assert int(rag["n_iter"][i]) == int(loop[i]["n_iter"][0]) and torch.equal(rag["cluster_features"][i], loop[i]["cluster_features"][0]), i
    n_iter = [int(v) for v in rag["n_iter"].cpu()]
    del loop, rag
    res_a = alternate({"kmeans_fit slide by slide": lambda: [kmeans_fit(x, 100) for x in slides],
                       "kmeans_fit_ragged(list)": lambda: kmeans_fit_ragged(slides, 100),
                       "kmeans_fit_ragged((X_cat, counts))": lambda: kmeans_fit_ragged((Xcat, counts), 100)},
                      S, args.rounds, args.calls, args.warmup)
    table(f"(a) {S} slides, {min(counts)}..{max(counts)} patches ({total} in all) x {DIM}; Lloyd iterations {min(n_iter)}..{max(n_iter)}; "
          f"the 4 GiB budget cuts the list into {len(plan)} calls; ragged results equal the slide-by-slide ones bit for bit",
          res_a, "kmeans_fit slide by slide")
    report["a"] = dict(counts=counts, calls_in_plan=len(plan), n_iter=n_iter, ms_per_slide=res_a)

    # (c) the same rows, cut as one 4000-patch slide among equal ones / as equal ones
    skew, flat = skewed_counts(total, S, min(4000, total - 100 * (S - 1)))
    res_c = alternate({"evenly spread": lambda: kmeans_fit_ragged((Xcat, flat), 100),
                       "one 4000-patch slide among the others": lambda: kmeans_fit_ragged((Xcat, skew), 100)},
                      S, args.rounds, args.calls, args.warmup)
    table(f"(c) the rows of (a) as {S} slides of {min(flat)}..{max(flat)} patches, and as one of {max(skew)} among {S - 1} of "
          f"{min(skew)}..{sorted(skew)[-2]} (calls: {len(ragged_plan(flat, DIM, 100, 4 << 30))} and {len(ragged_plan(skew, DIM, 100, 4 << 30))})",
          res_c, "evenly spread")
    report["c"] = dict(even=flat, skewed=skew, ms_per_slide=res_c)
    del slides, Xcat

    # (b) equal counts: the uniform batch against the ragged call
    Xb = torch.from_numpy(np.stack([synth.features_gmm(500 + i, 1000, DIM) for i in range(8)])).cuda()
    flat_b = Xb.view(8000, DIM)
    res_b = alternate({"kmeans_fit_batch": lambda: kmeans_fit_batch(Xb, 100),
                       "kmeans_fit_ragged((X_cat, counts))": lambda: kmeans_fit_ragged((flat_b, [1000] * 8), 100)},
                      8, args.rounds, max(args.calls, 10), max(args.warmup, 2))
    table(f"(b) 8 x 1000 x {DIM}", res_b, "kmeans_fit_batch")
    report["b"] = dict(ms_per_slide=res_b)

    lines.append(json.dumps(report))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
