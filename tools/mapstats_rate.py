"""Time of the device map statistics (sequoia_pub_amd.mapstats, csrc/mapstats.hip) beside the reference's own calls
(spatial_vis/gbm_celltype_analysis.py: DataFrame.mean(axis=1), one scipy.stats.percentileofscore per row, DataFrame.corr())
on one core, in ONE process:
    python tools/mapstats_rate.py [--seconds 0.3] [--rounds 5] [--out profiles/mapstats_rate.txt]
Shapes, all with n = 50 000 tiles (a config-5 slide):
    means        4 categories of 60 genes of an f32 table [n, 256]
    perc 4       the percentiles of the 4 f64 category means and the leading category (the cell-type map's step)
    perc 256     the percentiles of 256 f32 gene columns, ranked in place through a column list of a table [n, 512]
    corr 256     the correlation of the 256 columns of an f32 table [n, 256]
    corr 2048    the same with 2048 columns
Per shape two device paths, warmed up, then timed in `rounds` windows of about `seconds` each, the paths alternating, a host
clock around each window with a device synchronise at its end; the line shows the median window per call and the spread:
    resident     the call on tensors in device memory, results left there
    with copies  upload of the input table from pinned memory + the call + download of the result
The host side is timed ONCE per shape with the BLAS / OpenMP pools limited to one thread where threadpoolctl is installed.  The
means are timed in full.  The percentiles and the correlation are timed on a ROW SUBSET and EXTRAPOLATED by their law: the
reference makes one O(n) percentileofscore call per row against the full column, so `rows` calls are timed and scaled by
n / rows (and by the number of columns where only some are timed); DataFrame.corr() is O(n K^2), linear in n, so it is
timed on `rows` rows and scaled by n / rows.  Every extrapolated figure is marked as such.  The yardstick is the project's
usual one: a box allows 16 CPUs, so a device path earns its place where its time with copies is below the host's one-core
time / 16.  Prints one line per measurement and a last JSON line; --out also writes them to a file."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch
from scipy.stats import percentileofscore

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, mapstats  # noqa: E402

N = 50_000
HOST_CPUS = 16


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), "threadpoolctl: 1 thread"
    except ImportError:
        return contextlib.nullcontext(), f"threadpoolctl absent: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"


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
        for _ in range(2):
            fn()
        calls[name] = max(2, int(seconds * 1e3 / max(window_ms(fn, 2), 1e-3)))
    for _ in range(rounds):
        for name, fn in paths.items():
            windows[name].append(window_ms(fn, calls[name]))
    return windows, calls


def host_seconds(fn):
    limiter, how = one_thread()
    with limiter:
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0, how


def score2percentile(score, ref):                       # gbm_celltype_analysis.py:12-16
    if np.isnan(score):
        return score
    return percentileofscore(ref, score)


def host_percentile_rows(column, rows):
    """`rows` of the reference's per-row calls against the FULL column."""
    ref = np.asarray(column, dtype=np.float64)
    df = pd.DataFrame({"v": ref[:rows]})
    return df.apply(lambda row: score2percentile(row["v"], ref), axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rows", type=int, default=400, help="rows of the host's percentile and correlation subsets")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows_out = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def report(label, paths, host_s, how, law):
        windows, calls = timed_paths(paths, args.seconds, args.rounds)
        med = {k: statistics.median(v) for k, v in windows.items()}
        say(label)
        for name in windows:
            say(f"    {name:12s} {med[name]:10.4f} ms  (windows {min(windows[name]):.4f}..{max(windows[name]):.4f}, {calls[name]} calls each)")
        host_ms = host_s * 1e3
        met = med["with copies"] < host_ms / HOST_CPUS
        say(f"    host, one core ({how}): {host_s:.3f} s {law}; / {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.1f} ms; with copies "
            f"{host_ms / med['with copies']:.0f} x one core, {host_ms / HOST_CPUS / med['with copies']:.1f} x sixteen")
        say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'}")
        rows_out.append(dict(shape=label, resident_ms=round(med["resident"], 5), with_copies_ms=round(med["with copies"], 5),
                             host_s=round(host_s, 4), host_law=law, host_threads=how, condition_met=bool(met)))

    rs = np.random.default_rng(7)
    m = args.host_rows

    # ---- category means + the percentiles of the four means
    table = rs.random((N, 256), dtype=np.float32) * 6.0
    lists = [rs.permutation(256)[:60].tolist() for _ in range(4)]
    pinned = torch.from_numpy(table).pin_memory()
    resident = pinned.cuda()
    staged = torch.empty_like(resident)

    def means_copies():
        staged.copy_(pinned, non_blocking=True)
        return mapstats.category_means(staged, lists).cpu()

    frame = pd.DataFrame(table.astype(np.float64))
    host_s, how = host_seconds(lambda: [frame[c].mean(axis=1) for c in lists])
    report(f"means: 4 categories of 60 genes, table {N} x 256 f32", {"resident": lambda: mapstats.category_means(resident, lists),
                                                                     "with copies": means_copies}, host_s, how, "(in full)")
    means = mapstats.category_means(resident, lists)
    means_host = means.cpu().numpy()
    means_pinned = torch.from_numpy(means_host).pin_memory()
    means_staged = torch.empty_like(means)

    def perc4_copies():
        means_staged.copy_(means_pinned, non_blocking=True)
        p, first = mapstats.percentile_of_score(means_staged, return_argmax=True)
        return p.cpu(), first.cpu()

    sub_s, how = host_seconds(lambda: [host_percentile_rows(means_host[:, k], m) for k in range(4)])
    got = mapstats.percentile_of_score(means)[:m].cpu().numpy()
    want = np.stack([host_percentile_rows(means_host[:, k], m).values for k in range(4)], axis=1)
    assert np.array_equal(got, want), "device percentiles differ from scipy's on the timed rows"
    report(f"perc 4: percentiles and leading category of 4 f64 columns, n = {N}",
           {"resident": lambda: mapstats.percentile_of_score(means, return_argmax=True), "with copies": perc4_copies},
           sub_s * N / m, how, f"(EXTRAPOLATED: {m} of {N} per-row calls per column took {sub_s:.3f} s, x {N / m:.0f}; the timed rows equal the device's bit for bit)")
    del resident, staged, pinned

    # ---- 256 gene columns ranked in place
    wide = rs.random((N, 512), dtype=np.float32) * 6.0
    cols = np.sort(rs.permutation(512)[:256]).astype(np.int32)
    pinned = torch.from_numpy(wide).pin_memory()
    resident = pinned.cuda()
    staged = torch.empty_like(resident)
    cols_dev = torch.from_numpy(cols).cuda()

    def perc256_copies():
        staged.copy_(pinned, non_blocking=True)
        return mapstats.percentile_of_score(staged, cols=cols_dev).cpu()

    timed_cols = 2
    sub_s, how = host_seconds(lambda: [host_percentile_rows(wide[:, cols[k]], m) for k in range(timed_cols)])
    report(f"perc 256: 256 f32 gene columns of a table {N} x 512 through a column list",
           {"resident": lambda: mapstats.percentile_of_score(resident, cols=cols_dev), "with copies": perc256_copies},
           sub_s * (N / m) * (256 / timed_cols), how,
           f"(EXTRAPOLATED: {m} of {N} per-row calls of {timed_cols} of 256 columns took {sub_s:.3f} s, x {N / m:.0f} x {256 // timed_cols})")
    del resident, staged, pinned, wide
    torch.cuda.empty_cache()

    # ---- correlation
    for K in (256, 2048):
        table = (rs.standard_normal((N, K), dtype=np.float32) + rs.standard_normal((N, 1), dtype=np.float32) * 0.5)
        pinned = torch.from_numpy(table).pin_memory()
        resident = pinned.cuda()
        staged = torch.empty_like(resident)

        def corr_copies():
            staged.copy_(pinned, non_blocking=True)
            return mapstats.gene_correlation(staged).cpu()

        sub = pd.DataFrame(table[:m].astype(np.float64))
        kept = []
        sub_s, how = host_seconds(lambda: kept.append(sub.corr()))
        got = mapstats.gene_correlation(resident[:m]).cpu().numpy()
        worst = float(np.max(np.abs(got - kept[0].values)))
        assert worst <= 4 * m * 2.0 ** -53, worst
        report(f"corr {K}: correlation of {K} f32 columns, n = {N}", {"resident": lambda: mapstats.gene_correlation(resident),
                                                                     "with copies": corr_copies},
               sub_s * N / m, how, f"(EXTRAPOLATED: DataFrame.corr() of {m} of {N} rows took {sub_s:.3f} s, x {N / m:.0f}; on those rows the "
                                   f"device is within {worst:.1e} of it)")
        del resident, staged, pinned, table
        torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, n=N, host_rows=m, rows=rows_out)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
