"""Time of the device patch filter (patchgen.filter_patches, csrc/patchfilter.hip) beside the host filter it can replace
(patchgen.get_mask_image + scipy's binary_dilation + patchgen.is_low_contrast, numpy float64 on one core), in ONE process:
    python tools/patch_filter_rate.py [--seconds 1.0] [--rounds 3] [--host-tiles 12] [--out profiles/patch_filter_rate.txt]
Cases: 1024 tiles of 256 x 256 (the default patch) and 256 tiles of 512 x 512 (the 40x read), each a mix of tissue-like,
blank and noise tiles in turn.  Per case two device paths -- the filter on tiles already in device memory, and the upload
from pinned host memory followed by the filter (what extract_patches(device=...) pays per chunk) -- and the filter on blank
and on one-colour tiles alone (the worst cases of the LDS histograms), warmed up, then timed
in `rounds` windows of about `seconds` each, the paths alternating, HIP events around every window; the line shows the
median window per tile and the spread.  The host filter is timed on `--host-tiles` tiles of the same mix with the BLAS /
OpenMP pools of the process limited to one thread where threadpoolctl is installed (the filter's own numpy code is
single-threaded; only the luminance product goes through BLAS), and the device decisions are compared with the host's on
those tiles.  The yardstick: a box that allows 16 CPUs can run 16 host filters side by side, so the device path earns its
place where its per-tile time with the upload is below the host's per-tile time / 16.  Prints one line per case and path
and a last JSON line; --out also writes them to a file."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.ndimage import binary_dilation

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, patchgen  # noqa: E402

CASES = [(1024, 256), (256, 512)]
HOST_CPUS = 16


def tile(size, kind, seed):
    """kind 0: paper with a band of tissue-coloured pixels; 1: blank paper; 2: uniform noise."""
    rs = np.random.RandomState(seed)
    if kind == 2:
        return rs.randint(0, 256, (size, size, 3)).astype(np.uint8)
    img = np.full((size, size, 3), 242, dtype=np.float64) + rs.randn(size, size, 3) * 2
    if kind == 0:
        x0, wide = int(rs.randint(0, size // 2)), int(rs.randint(size // 4, size // 2))
        img[:, x0:x0 + wide] = np.array([190, 110, 160]) + rs.randn(size, wide, 3) * 25
    return np.clip(img, 0, 255).astype(np.uint8)


def host_keep(img):
    tissue = binary_dilation(patchgen.get_mask_image(img), iterations=3)
    return bool(tissue.sum() > 0.2 * tissue.size and not patchgen.is_low_contrast(img))


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), "threadpoolctl: 1 thread"
    except ImportError:
        return contextlib.nullcontext(), f"threadpoolctl absent: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-tiles", type=int, default=12, help="tiles the host filter is timed on, per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for n, size in CASES:
        distinct = np.stack([tile(size, i % 3, 100 * size + i) for i in range(48)])
        pinned = torch.from_numpy(distinct[np.arange(n) % 48]).pin_memory()
        x = pinned.cuda()
        dev_buf = torch.empty_like(x)

        def upload_and_filter():
            dev_buf.copy_(pinned, non_blocking=True)
            return patchgen.filter_patches(dev_buf)

        # the histograms' worst cases, apart from the mix: blank paper alone (kind 1) and tiles of one colour each, where every
        # pixel of a tile goes to one bin of every histogram
        blank = torch.from_numpy(distinct[1::3][np.arange(n) % 16]).cuda()
        flat = torch.from_numpy(np.broadcast_to(distinct[:, :1, :1], distinct.shape)[np.arange(n) % 48].copy()).cuda()
        paths = {"filter (tiles on the device)": lambda: patchgen.filter_patches(x), "upload from pinned memory + filter": upload_and_filter,
                 "filter, blank tiles only": lambda: patchgen.filter_patches(blank), "filter, one-colour tiles only": lambda: patchgen.filter_patches(flat)}
        calls, windows, keep = {}, {k: [] for k in paths}, {}
        for name, fn in paths.items():
            for _ in range(3):
                keep[name] = fn()
            torch.cuda.synchronize()
            calls[name] = max(3, int(args.seconds * 1e3 / window_ms(fn, 3)))
        for _ in range(args.rounds):
            for name, fn in paths.items():
                windows[name].append(window_ms(fn, calls[name]))
        a, b = (keep[k].cpu().numpy() for k in list(paths)[:2])
        assert np.array_equal(a, b) and not keep["filter, blank tiles only"].any() and not keep["filter, one-colour tiles only"].any()
        limiter, how = one_thread()
        with limiter:
            host_keep(distinct[0])
            t0 = time.perf_counter()
            want = [host_keep(distinct[i]) for i in range(args.host_tiles)]
            host_ms = (time.perf_counter() - t0) * 1e3 / args.host_tiles
        agree = int(sum(bool(a[i]) == want[i] for i in range(args.host_tiles)))
        case = f"{n} x {size} x {size}"
        for name in paths:
            us = statistics.median(windows[name]) * 1e3 / n
            row = dict(case=case, path=name, us_per_tile=round(us, 3), us_min=round(min(windows[name]) * 1e3 / n, 3),
                       us_max=round(max(windows[name]) * 1e3 / n, 3), ms_per_call=round(statistics.median(windows[name]), 4),
                       calls_per_window=calls[name], gb_per_s=round(3.0 * size * size / us / 1e3, 1))
            rows.append(row)
            say(f"{case:>18s}  {name:36s} {us:9.3f} us / tile  (windows {row['us_min']:.3f}..{row['us_max']:.3f}, {calls[name]} calls each)"
                f"  {row['gb_per_s']:7.1f} GB/s of uint8 pixels")
        with_upload = statistics.median(windows["upload from pinned memory + filter"]) * 1e3 / n
        met = with_upload < host_ms * 1e3 / HOST_CPUS
        say(f"{'':>18s}  host filter, one core ({how}): {host_ms:.2f} ms / tile over {args.host_tiles} tiles; / {HOST_CPUS} CPUs = "
            f"{host_ms * 1e3 / HOST_CPUS:.1f} us; device with upload {with_upload:.2f} us = {host_ms * 1e3 / with_upload:.0f} x one core, "
            f"{host_ms * 1e3 / HOST_CPUS / with_upload:.1f} x sixteen: condition {'met' if met else 'NOT met'}; "
            f"{int(a.sum())} of {n} tiles kept, decisions equal the host's on {agree} of {args.host_tiles}")
        rows.append(dict(case=case, host_ms_per_tile=round(host_ms, 3), host_tiles=args.host_tiles, host_threads=how,
                         host_us_per_tile_over_16=round(host_ms * 1e3 / HOST_CPUS, 2), device_with_upload_us=round(with_upload, 3),
                         condition_met=bool(met), kept=int(a.sum()), decisions_equal=agree))
        del x, dev_buf, pinned, blank, flat
        torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, rows=rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
