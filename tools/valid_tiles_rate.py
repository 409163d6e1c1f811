"""Time of the device valid-tile grid (patchgen.valid_tile_grid, csrc/tilegrid.hip; cli.visualize.valid_tiles_device) beside
the host loop it can replace (cli.visualize.valid_tiles: scipy's binary_dilation per grid tile, one core), in ONE process:
    python tools/valid_tiles_rate.py [--seconds 0.5] [--rounds 5] [--out profiles/valid_tiles_rate.txt]
Shapes: a slide of 100 000 x 80 000 pixels with (a) a mask downsampled by 32 and a read size of 256 (windows of 8 x 8,
121 680 grid tiles), (b) the same mask and a read size of 512, a 40x slide (16 x 16, 30 420 tiles), (c) a mask downsampled
by 16 and a read size of 256 (16 x 16, 121 680 tiles); the mask is synthetic, elliptic blobs of tissue over about a third of
it with specks around them.  Per shape three device paths, warmed up, then timed in `rounds` windows of about `seconds` each,
the paths alternating, a host clock around each window with a device synchronise at its end (every path ends in a copy or
a nonzero that waits for the device anyway); the line shows the median window per call and the spread:
    resident     valid_tile_grid on a mask in device memory + torch.nonzero: kernel and index build, no copies
    with copies  upload of the uint8 mask from pinned memory + the same + download of the indices
    as the CLI   valid_tiles_device(numpy mask): also the mask != 0 pass into freshly pinned memory and the DataFrame
The host loop is timed once per shape with the BLAS / OpenMP pools limited to one thread where threadpoolctl is installed,
and its frame is compared with the device's (pd.testing.assert_frame_equal).  The yardstick is the per-tile filter's: a box
allows 16 CPUs, so the device path earns its place where its time with copies is below the host's one-core time / 16.
Prints one line per measurement and a last JSON line; --out also writes them to a file."""
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, patchgen  # noqa: E402
from sequoia_pub_amd.cli import visualize  # noqa: E402

SLIDE = (100_000, 80_000)
SHAPES = [("ds 32, read 256", 32, 256), ("ds 32, read 512", 32, 512), ("ds 16, read 256", 16, 256)]
HOST_CPUS = 16


def synthetic_mask(mask_w, mask_h, seed):
    rs = np.random.default_rng(seed)
    xx, yy = np.ogrid[:mask_w, :mask_h]
    on = np.zeros((mask_w, mask_h), dtype=bool)
    for _ in range(12):
        cx, cy = rs.integers(0, mask_w), rs.integers(0, mask_h)
        rx, ry = rs.integers(mask_w // 24, mask_w // 7), rs.integers(mask_h // 24, mask_h // 7)
        on |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1.0
    on |= rs.random((mask_w, mask_h)) < 0.01
    return on


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
    """{name: [ms per call of each window]} with the paths alternating; every path warmed up first."""
    calls, windows = {}, {k: [] for k in paths}
    for name, fn in paths.items():
        for _ in range(3):
            fn()
        calls[name] = max(3, int(seconds * 1e3 / max(window_ms(fn, 3), 1e-3)))
    for _ in range(rounds):
        for name, fn in paths.items():
            windows[name].append(window_ms(fn, calls[name]))
    return windows, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="only the first so many shapes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for label, ds, p in SHAPES[:args.shapes]:
        mask = synthetic_mask(SLIDE[0] // ds, SLIDE[1] // ds, 100 * ds + p)
        got_ds, pm, n_col, n_row = patchgen.tile_grid_geometry(mask.shape, SLIDE, p)
        assert got_ds == ds
        pinned = torch.from_numpy(mask.view(np.uint8)).pin_memory()
        resident = pinned.cuda()
        staged = torch.empty_like(resident)

        def with_copies():
            staged.copy_(pinned, non_blocking=True)
            return torch.nonzero(patchgen.valid_tile_grid(staged, SLIDE, p)).cpu()

        paths = {"resident": lambda: torch.nonzero(patchgen.valid_tile_grid(resident, SLIDE, p)),
                 "with copies": with_copies,
                 "as the CLI": lambda: visualize.valid_tiles_device(mask, SLIDE, p, "cuda:0")}
        windows, calls = timed_paths(paths, args.seconds, args.rounds)
        frame = visualize.valid_tiles_device(mask, SLIDE, p, "cuda:0")
        limiter, how = one_thread()
        with limiter:
            t0 = time.perf_counter()
            want = visualize.valid_tiles(mask, SLIDE, p)
            host_s = time.perf_counter() - t0
        pd.testing.assert_frame_equal(frame, want)
        assert np.array_equal(with_copies().numpy() * p, want[["xcoord", "ycoord"]].values)
        shape = f"mask {mask.shape[0]} x {mask.shape[1]} ({label}), windows of {pm} x {pm}, {n_col * n_row} grid tiles, {len(want)} valid"
        say(shape)
        med = {k: statistics.median(v) for k, v in windows.items()}
        for name in windows:
            say(f"    {name:12s} {med[name]:9.4f} ms  (windows {min(windows[name]):.4f}..{max(windows[name]):.4f}, {calls[name]} calls each)")
            rows.append(dict(shape=label, path=name, ms_per_call=round(med[name], 5), ms_min=round(min(windows[name]), 5),
                             ms_max=round(max(windows[name]), 5), calls_per_window=calls[name]))
        host_ms = host_s * 1e3
        met, met_cli = med["with copies"] < host_ms / HOST_CPUS, med["as the CLI"] < host_ms / HOST_CPUS
        say(f"    host, one core ({how}): valid_tiles {host_s:.3f} s, once; / {HOST_CPUS} CPUs = {host_ms / HOST_CPUS:.1f} ms; with copies "
            f"{host_ms / med['with copies']:.0f} x one core, {host_ms / HOST_CPUS / med['with copies']:.1f} x sixteen; frames equal")
        say(f"    with copies below host / {HOST_CPUS} CPUs: {'met' if met else 'not met'}  (the whole call as the CLI makes it: "
            f"{'met' if met_cli else 'not met'})")
        rows.append(dict(shape=label, mask=list(mask.shape), pm=pm, grid_tiles=n_col * n_row, valid_tiles=len(want), host_s=round(host_s, 4),
                         host_threads=how, host_ms_over_16=round(host_ms / HOST_CPUS, 3), with_copies_ms=round(med["with copies"], 5),
                         as_cli_ms=round(med["as the CLI"], 5), condition_met=bool(met), condition_met_as_cli=bool(met_cli), frames_equal=True))
        del resident, staged, pinned
        torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, rows=rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
