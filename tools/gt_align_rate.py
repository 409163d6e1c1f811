"""Time of the device ground-truth alignment (sequoia_pub_amd.gtalign, csrc/gtalign.hip) beside the reference's own
get_average and median_filter (spatial_vis/get_emd.py) on one core, in ONE process:
    python tools/gt_align_rate.py --reference <the reference's spatial_vis folder> [--seconds 0.3] [--rounds 5] [--out profiles/gt_align_rate.txt]
Workloads: a full grid of 50 000 tiles (250 x 200, pitch 224) and one of 2000 tiles (50 x 40) -- the regime where one thread
per tile is thinnest -- each against 4992 spots (one Visium slide), for 1 gene and for 64 genes.
Per workload the four library entries and the whole align_ground_truth, two device paths each, warmed up, then timed in
`rounds` windows of about `seconds` each, the paths alternating, HIP events around each window; the line shows the median
window per call and the spread:
    resident     the call on tensors in device memory, results left there (align_ground_truth returns DataFrames, so its
                 downloads are inside both paths)
    with copies  upload of the call's inputs from pinned memory + the call + download of its result
The host side is the reference's LITERAL functions, imported from --reference (cv2, ot and scanpy stubbed), timed once with
the BLAS / OpenMP pools limited to one thread where threadpoolctl is installed, on `host_rows` of the rows against the FULL
frames, and EXTRAPOLATED linearly in the row count and in the gene count (the reference repeats both functions for every
gene); the timed rows are compared with the device's bit for bit.  Every extrapolated figure is marked as such.  The
yardstick is the project's usual one: a box allows 16 CPUs, so a device path earns its place where its time with copies is
below the host's one-core time / 16.  Without --reference only the device times are reported.  Prints one line per
measurement and a last JSON line; --out also writes them to a file."""
import argparse
import contextlib
import importlib.util
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, gtalign  # noqa: E402

N_SPOTS = 4992
HOST_CPUS = 16
PITCH = 224.0
NUM_TILES = 4


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


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), "threadpoolctl: 1 thread"
    except ImportError:
        return contextlib.nullcontext(), f"threadpoolctl absent: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"


def window_ms(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


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


def slide(grid_w, grid_h, genes, rs):
    """A full grid of tiles in permuted row order, N_SPOTS spots over its area, f32 predictions and f32 expression."""
    n = grid_w * grid_h
    order = rs.permutation(n)
    xtf, ytf = (np.arange(n) // grid_h)[order], (np.arange(n) % grid_h)[order]
    return dict(n=n, xtf=xtf.astype(np.int32), ytf=ytf.astype(np.int32), xcoord=1000.0 + PITCH * xtf, ycoord=500.0 + PITCH * ytf,
                spot_x=1000.0 + rs.uniform(0.0, PITCH * grid_w, N_SPOTS), spot_y=500.0 + rs.uniform(0.0, PITCH * grid_h, N_SPOTS),
                expr=rs.standard_normal((N_SPOTS, genes)).astype(np.float32), pred=(rs.random((n, genes)) * 4.0).astype(np.float32),
                names=[f"g{i}" for i in range(genes)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the folder that holds the reference's get_emd.py (its spatial_vis)")
    ap.add_argument("--seconds", type=float, default=0.3, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host_rows", type=int, default=200, help="rows of the host's subsets")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    ref = load_get_emd(args.reference) if args.reference else None
    lines, rows_out = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def report(label, paths, host_ms=None, law=""):
        windows, calls = timed_paths(paths, args.seconds, args.rounds)
        med = {k: statistics.median(v) for k, v in windows.items()}
        say(label)
        for name in windows:
            say(f"    {name:12s} {med[name]:10.4f} ms  (windows {min(windows[name]):.4f}..{max(windows[name]):.4f}, {calls[name]} calls each)")
        row = dict(shape=label, resident_ms=round(med["resident"], 5), with_copies_ms=round(med["with copies"], 5))
        if host_ms is not None:
            met = med["with copies"] < host_ms / HOST_CPUS
            factor = host_ms / HOST_CPUS / med["with copies"]
            say(f"    host, one core: {host_ms / 1e3:.2f} s {law}; / {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.1f} ms; with copies "
                f"{host_ms / med['with copies']:.0f} x one core")
            say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'} by a factor of {factor if met else 1 / factor:.1f}")
            row.update(host_s=round(host_ms / 1e3, 4), host_law=law, condition_met=bool(met), factor=round(factor, 2))
        rows_out.append(row)
        return med

    rs = np.random.default_rng(11)
    m = args.host_rows
    for grid_w, grid_h in ((250, 200), (50, 40)):
        for genes in (1, 64):
            s = slide(grid_w, grid_h, genes, rs)
            n = s["n"]
            tag = f"{n} tiles x {N_SPOTS} spots, {genes} gene{'s' if genes > 1 else ''}"
            pinned = {k: torch.from_numpy(np.ascontiguousarray(s[k])).pin_memory() for k in ("xtf", "ytf", "xcoord", "ycoord", "spot_x", "spot_y", "expr", "pred")}
            dev = {k: v.cuda() for k, v in pinned.items()}
            staged = {k: torch.empty_like(v) for k, v in dev.items()}

            def up(*keys):
                for k in keys:
                    staged[k].copy_(pinned[k], non_blocking=True)
                return [staged[k] for k in keys]

            idx = gtalign.nearest_spots(dev["xcoord"], dev["ycoord"], dev["spot_x"], dev["spot_y"], num_tiles=NUM_TILES)
            gt = gtalign.spot_means(idx, dev["expr"])
            filt = gtalign.median_filter(gt, dev["xtf"], dev["ytf"], nan_absent=True)
            gt_pinned = gt.cpu().pin_memory()
            gt_staged = torch.empty_like(gt)
            idx_pinned = idx.cpu().pin_memory()
            idx_staged = torch.empty_like(idx)

            # ---- the host's literal functions on `m` rows of the full frames
            host = None
            if ref is not None:
                limiter, how = one_thread()
                df = pd.DataFrame({"x": s["spot_x"], "y": s["spot_y"]})
                df["gene_expr"] = s["expr"][:, 0]
                gt_host = gt.cpu().numpy()
                df2 = pd.DataFrame({"xcoord_tf": s["xtf"], "ycoord_tf": s["ytf"], "ground_truth": gt_host[:, 0]})
                with limiter:
                    t0 = time.perf_counter()
                    ga = [ref.get_average(s["xcoord"][i], s["ycoord"][i], df, NUM_TILES) for i in range(m)]
                    t_ga = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    mf = [ref.median_filter(df2, "ground_truth", s["xtf"][i], s["ytf"][i], 1) for i in range(m)]
                    t_mf = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    uq = [len(np.unique(gt_host[:, c])) for c in range(genes)]
                    t_uq = time.perf_counter() - t0
                assert np.array_equal(np.array(ga), gt_host[:m, 0]), "device means differ from get_average on the timed rows"
                assert np.array_equal(np.array(mf), filt[:m, 0].cpu().numpy()), "device medians differ from median_filter on the timed rows"
                assert uq == gtalign.count_unique(gt).cpu().numpy().tolist(), "device counts differ from np.unique"
                scale = n / m * genes
                law = f"(EXTRAPOLATED: {m} of {n} rows of 1 of {genes} genes, x {n / m:.0f} x {genes}; the timed rows equal the device's bit for bit; {how})"
                host = dict(ga=t_ga * scale * 1e3, mf=t_mf * scale * 1e3, uq=t_uq * 1e3, law=law,
                            ga_call=t_ga / m * 1e3, mf_call=t_mf / m * 1e3)
                say(f"{tag}: host get_average {host['ga_call']:.3f} ms a call, median_filter {host['mf_call']:.3f} ms a call, one core")

            def ns_copies():
                a = up("xcoord", "ycoord", "spot_x", "spot_y")
                return gtalign.nearest_spots(*a, num_tiles=NUM_TILES).cpu()

            ns = report(f"nearest spots: {n} tiles x {N_SPOTS} spots, k = {NUM_TILES}",
                        {"resident": lambda: gtalign.nearest_spots(dev["xcoord"], dev["ycoord"], dev["spot_x"], dev["spot_y"], num_tiles=NUM_TILES),
                         "with copies": ns_copies})

            def means_copies():
                idx_staged.copy_(idx_pinned, non_blocking=True)
                return gtalign.spot_means(idx_staged, up("expr")[0]).cpu()

            me = report(f"spot means: {tag}", {"resident": lambda: gtalign.spot_means(idx, dev["expr"]), "with copies": means_copies})
            if host:
                both = ns["with copies"] + me["with copies"]
                met = both < host["ga"] / HOST_CPUS
                factor = host["ga"] / HOST_CPUS / both
                say(f"ground truth (nearest spots + spot means, with copies {both:.3f} ms) against get_average: host, one core "
                    f"{host['ga'] / 1e3:.1f} s {host['law']}; / {HOST_CPUS} CPUs = {host['ga'] / HOST_CPUS:.0f} ms: "
                    f"{'met' if met else 'not met'} by a factor of {factor if met else 1 / factor:.0f}")
                rows_out.append(dict(shape=f"ground truth: {tag}", with_copies_ms=round(both, 5), host_s=round(host["ga"] / 1e3, 3),
                                     condition_met=bool(met), factor=round(factor, 1)))

            def mf_copies():
                gt_staged.copy_(gt_pinned, non_blocking=True)
                return gtalign.median_filter(gt_staged, *up("xtf", "ytf"), nan_absent=True).cpu()

            report(f"median filter r = 1: {tag}", {"resident": lambda: gtalign.median_filter(gt, dev["xtf"], dev["ytf"], nan_absent=True),
                                                  "with copies": mf_copies}, host and host["mf"], host["law"] if host else "")

            def uq_copies():
                gt_staged.copy_(gt_pinned, non_blocking=True)
                return gtalign.count_unique(gt_staged).cpu()

            report(f"count unique: {tag}", {"resident": lambda: gtalign.count_unique(gt), "with copies": uq_copies},
                   host and host["uq"], "(np.unique of every column, in full)" if host else "")

            def align(t):
                return gtalign.align_ground_truth(t["pred"], s["names"], t["xcoord"], t["ycoord"], t["xtf"], t["ytf"], t["spot_x"], t["spot_y"],
                                                  t["expr"], s["names"], num_tiles=NUM_TILES)

            def align_copies():
                up(*staged.keys())
                return align(staged)

            report(f"align_ground_truth: {tag}", {"resident": lambda: align(dev), "with copies": align_copies},
                   host and host["ga"] + host["mf"],
                   host["law"].replace("(EXTRAPOLATED:", "(EXTRAPOLATED, get_average + median_filter only, the percentiles left out:") if host else "")
            del pinned, dev, staged, idx, gt, filt
            torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, n_spots=N_SPOTS, host_rows=m, rows=rows_out)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
