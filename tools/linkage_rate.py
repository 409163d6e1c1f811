"""Time of the device average-linkage clustering (sequoia_pub_amd.mapstats.linkage_average, csrc/linkage.hip) beside scipy's
pdist + linkage(method='average') on one core, in ONE process:
    python tools/linkage_rate.py [--seconds 0.3] [--rounds 5] [--sizes 256 1024 2048 4096] [--out profiles/linkage_rate.txt]
Per K a symmetric f64 matrix [K, K] of noise (M = K features, as the gene correlation map is clustered).  Two device paths,
warmed up, then timed in `rounds` windows of about `seconds` each, the paths alternating, a host clock around each window
with a device synchronise at its end; the line shows the median window per call and the spread:
    resident     linkage_average on a matrix in device memory, Z and the leaves left there (the status words are downloaded:
                 that is the call)
    with copies  upload of the matrix from pinned memory + the call + download of Z and the leaves
and the distance stage alone (row_distances, resident) with the rate it reaches on its K^2 M / 2 pairs x features, two rounded
operations each (a product and a sum; the difference comes on top).  The host's pdist and linkage are timed apart, each
repeated for about `--host_seconds` (at least once, at most `--host_repeats` times) and reported by its FASTEST run with
the number of runs; the device's Z and leaves are compared with scipy's bit for bit in the same run.  The yardstick is the project's usual
one: a box allows 16 CPUs, so the device path earns its place where its time with copies is below the host's one-core time
/ 16.  Prints one line per measurement and a last JSON line; --out also writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.cluster.hierarchy import leaves_list, linkage
from scipy.spatial.distance import pdist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, mapstats  # noqa: E402

HOST_CPUS = 16


def window_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def timed_paths(paths, seconds, rounds):
    calls, windows = {}, {k: [] for k in paths}
    for name, fn in paths.items():
        fn()
        calls[name] = max(1, int(seconds * 1e3 / max(window_ms(fn, 1), 1e-3)))
    for _ in range(rounds):
        for name, fn in paths.items():
            windows[name].append(window_ms(fn, calls[name]))
    return windows, calls


def best_of(fn, seconds, most):
    """(result, fastest run in seconds, runs): fn repeated until `seconds` have passed, at least once and at most `most` times."""
    times, t_start = [], time.perf_counter()
    while not times or (len(times) < most and time.perf_counter() - t_start < seconds):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, min(times), len(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 2048, mapstats.MAX_LINK_ROWS])
    ap.add_argument("--host_seconds", type=float, default=1.0, help="about how long each host stage is repeated")
    ap.add_argument("--host_repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows_out = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    rs = np.random.RandomState(11)
    for K in args.sizes:
        a = rs.standard_normal((K, K))
        a = (a + a.T) / 2.0
        pinned = torch.from_numpy(a).pin_memory()
        resident = pinned.cuda()
        staged = torch.empty_like(resident)

        def with_copies():
            staged.copy_(pinned, non_blocking=True)
            Z, leaves = mapstats.linkage_average(staged)
            return Z.cpu(), leaves.cpu()

        d, host_pdist, runs_pdist = best_of(lambda: pdist(a, "euclidean"), args.host_seconds, args.host_repeats)
        want, host_link, runs_link = best_of(lambda: linkage(d, method="average"), args.host_seconds, args.host_repeats)
        Z, leaves = mapstats.linkage_average(resident)
        equal = Z.cpu().numpy().tobytes() == want.tobytes() and leaves.cpu().numpy().tolist() == leaves_list(want).tolist()
        windows, calls = timed_paths({"resident": lambda: mapstats.linkage_average(resident), "with copies": with_copies,
                                      "distances": lambda: mapstats.row_distances(resident)}, args.seconds, args.rounds)
        med = {k: statistics.median(v) for k, v in windows.items()}
        say(f"K = {K}: average linkage of a {K} x {K} f64 matrix (Z and leaves {'EQUAL' if equal else 'DIFFER FROM'} scipy's bit for bit)")
        for name in windows:
            say(f"    {name:12s} {med[name]:10.4f} ms  (windows {min(windows[name]):.4f}..{max(windows[name]):.4f}, {calls[name]} calls each)")
        ops = float(K) * K * K
        say(f"    distances: K^2 M = {ops:.3g} rounded products and sums in {med['distances']:.4f} ms = {ops / med['distances'] / 1e6:.1f} Gop/s "
            "(separately rounded, features in order: no FMA, no matrix pipe)")
        host_ms = (host_pdist + host_link) * 1e3
        met = med["with copies"] < host_ms / HOST_CPUS
        say(f"    host, one core: pdist {host_pdist * 1e3:.2f} ms (fastest of {runs_pdist}) + linkage {host_link * 1e3:.2f} ms (fastest of {runs_link}) = "
            f"{host_ms:.2f} ms; / {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.2f} ms; with copies "
            f"{host_ms / med['with copies']:.1f} x one core, {host_ms / HOST_CPUS / med['with copies']:.2f} x sixteen")
        say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'}")
        rows_out.append(dict(K=K, resident_ms=round(med["resident"], 5), with_copies_ms=round(med["with copies"], 5),
                             distances_ms=round(med["distances"], 5), host_pdist_ms=round(host_pdist * 1e3, 3), host_linkage_ms=round(host_link * 1e3, 3), host_runs=[runs_pdist, runs_link],
                             equal_to_scipy=bool(equal), condition_met=bool(met)))
        del resident, staged, pinned
        torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, rows=rows_out)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
