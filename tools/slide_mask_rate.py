"""Time of the device slide mask (patchgen.slide_mask, csrc/slidemask.hip) beside the host code it can replace
(patchgen.get_mask_image on the transposed level image + scipy's three dilations and three erosions, numpy float64 on one
core), in ONE process:
    python tools/slide_mask_rate.py [--seconds 1.0] [--rounds 3] [--out profiles/slide_mask_rate.txt]
Shapes: level images of 1536 x 2048, 3072 x 4096 and 6144 x 8192 pixels; content: tissue-like (paper with blobs of
tissue-coloured pixels), blank paper and uniform noise.  Per shape and content two device paths -- the call on an image
already in device memory, and upload from pinned memory + call(transpose=True) + download of the bool [W, H] mask (what
extract_patches(slide_mask="device") pays per slide) -- warmed up, then timed in `rounds` windows of about `seconds` each,
the paths alternating, HIP events around every window; the line shows the median window per call and the spread.  The host
path is timed once per shape and content (`--host-max-pixels` bounds the shapes it runs on in full; beyond it only the mask
without the closing is computed, on the tissue-like image, for the comparison) with the BLAS / OpenMP pools limited to one
thread where threadpoolctl is installed.  Device and host results of the same run are compared: thresholds, counts and every mask bit on the shapes
the host ran in full, thresholds and the raw count beyond.  The yardstick is the per-tile filter's: a box allows 16 CPUs,
so the device path earns its place where its time with upload and download is below the host's one-core time / 16.
Also reported: the rate of image bytes read (three sweeps x 3 bytes per pixel over the resident call's time) as a share of
the achievable HBM bandwidth, and the time of the call on a 64 x 64 image, which is the floor set by the launches and the
one-lane Otsu walk (2 x 256 sequential steps).  Which kernel dominates comes from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with --profile-pass (one shape, no host path).
Prints one line per measurement and a last JSON line; --out also writes them to a file."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.ndimage import binary_dilation, binary_erosion

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, patchgen  # noqa: E402

SHAPES = [(1536, 2048), (3072, 4096), (6144, 8192)]
KINDS = ["tissue-like", "blank", "noise"]
HOST_CPUS = 16
HBM_ACHIEVABLE_GBS = 6300.0          # what a streaming read reaches on an MI355X (8 TB/s nominal)


def level_image(h, w, kind, seed):
    """tissue-like: paper (242 +- 2) with elliptic blobs of tissue-coloured pixels (+- 25) over about a third of it."""
    rs = np.random.default_rng(seed)
    if kind == "noise":
        return rs.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img = (242.0 + rs.standard_normal((h, w, 3), dtype=np.float32) * 2).clip(0, 255).astype(np.uint8)
    if kind == "tissue-like":
        yy, xx = np.ogrid[:h, :w]
        on = np.zeros((h, w), dtype=bool)
        for _ in range(12):
            cy, cx, ry, rx = rs.integers(0, h), rs.integers(0, w), rs.integers(h // 12, h // 4), rs.integers(w // 12, w // 4)
            on |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        tissue = (np.array([190, 110, 160], dtype=np.float32) + rs.standard_normal((int(on.sum()), 3), dtype=np.float32) * 25)
        img[on] = tissue.clip(0, 255).astype(np.uint8)
    return img


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


def timed_paths(paths, seconds, rounds):
    """{name: [ms per call of each window]} with the paths alternating; every path warmed up first."""
    calls, windows = {}, {k: [] for k in paths}
    for name, fn in paths.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(seconds * 1e3 / max(window_ms(fn, 3), 1e-3)))
    for _ in range(rounds):
        for name, fn in paths.items():
            windows[name].append(window_ms(fn, calls[name]))
    return windows, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-max-pixels", type=int, default=3072 * 4096, help="largest image the host path is run on in full")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="only the first so many shapes")
    ap.add_argument("--profile-pass", action="store_true", help="a short run for rocprofv3: the 3072 x 4096 tissue-like image, device call only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if args.profile_pass:
        x = torch.from_numpy(level_image(3072, 4096, "tissue-like", 1)).cuda()
        for _ in range(20):
            patchgen.slide_mask(x, transpose=True)
        torch.cuda.synchronize()
        return

    # the floor: launches and the sequential Otsu walk, on an image of one chunk
    small = torch.from_numpy(level_image(64, 64, "noise", 3)).cuda()
    w, c = timed_paths({"floor": lambda: patchgen.slide_mask(small, transpose=True)}, min(args.seconds, 0.5), args.rounds)
    floor_us = statistics.median(w["floor"]) * 1e3
    say(f"{'64 x 64':>12s} {'noise':12s} call on a resident image {floor_us:9.1f} us  (windows {min(w['floor']) * 1e3:.1f}..{max(w['floor']) * 1e3:.1f}, "
        f"{c['floor']} calls each): memset + 6 launches, the one-lane Otsu walk among them")
    rows.append(dict(shape="64 x 64", kind="noise", path="resident", us_per_call=round(floor_us, 2)))

    for h, wd in SHAPES[:args.shapes]:
        for kind in KINDS:
            img = level_image(h, wd, kind, 7 * h + KINDS.index(kind))
            pinned = torch.from_numpy(img).pin_memory()
            x = pinned.cuda()
            dev_buf = torch.empty_like(x)
            host_out = torch.empty((wd, h), dtype=torch.bool).pin_memory()

            def end_to_end():
                dev_buf.copy_(pinned, non_blocking=True)
                host_out.copy_(patchgen.slide_mask(dev_buf, transpose=True), non_blocking=True)

            windows, calls = timed_paths({"call on a resident image": lambda: patchgen.slide_mask(x, transpose=True),
                                          "pinned upload + call + download": end_to_end}, args.seconds, args.rounds)
            closed, raw, stats = patchgen.slide_mask(x, transpose=True, return_raw=True, return_stats=True)
            end_to_end()
            torch.cuda.synchronize()
            closed, raw, stats = closed.cpu().numpy(), raw.cpu().numpy(), stats.cpu().numpy()
            assert np.array_equal(host_out.numpy(), closed)

            full = h * wd <= args.host_max_pixels
            if not full and kind != "tissue-like":                        # beyond the bound the host runs on one content only
                for name in windows:
                    med = statistics.median(windows[name])
                    say(f"{h} x {wd:<5d} {kind:12s} {name:32s} {med:9.3f} ms  (windows {min(windows[name]):.3f}..{max(windows[name]):.3f}, "
                        f"{calls[name]} calls each; host path not run)")
                    rows.append(dict(shape=f"{h} x {wd}", kind=kind, path=name, ms_per_call=round(med, 4), ms_min=round(min(windows[name]), 4),
                                     ms_max=round(max(windows[name]), 4), calls_per_window=calls[name]))
                del x, dev_buf, pinned, host_out
                torch.cuda.empty_cache()
                continue
            limiter, how = one_thread()
            with limiter:
                t_img = np.transpose(img, (1, 0, 2))                      # the [x, y] view get_mask hands over
                t0 = time.perf_counter()
                want_raw = patchgen.get_mask_image(t_img)
                t1 = time.perf_counter()
                want_closed = binary_erosion(binary_dilation(want_raw, iterations=3), iterations=3) if full else None
                t2 = time.perf_counter()
                want_thr = [float(patchgen.threshold_otsu(img[:, :, ch])) for ch in range(3)] + [float(patchgen.threshold_otsu(patchgen.saturation(img)))]
            mask_s, close_s = t1 - t0, (t2 - t1) if full else float("nan")
            thr_equal = bool(np.array_equal(stats[:4], np.array(want_thr)))
            raw_equal = bool(np.array_equal(raw, want_raw)) and stats[4] == want_raw.sum()
            closed_equal = (bool(np.array_equal(closed, want_closed)) and stats[5] == want_closed.sum()) if full else None

            shape = f"{h} x {wd}"
            med = {k: statistics.median(v) for k, v in windows.items()}
            for name in windows:
                gbs = 9.0 * h * wd / (med[name] * 1e-3) / 1e9
                extra = f"  {gbs:7.1f} GB/s of image bytes read (3 sweeps x 3 B) = {100 * gbs / HBM_ACHIEVABLE_GBS:.1f} % of {HBM_ACHIEVABLE_GBS:.0f} GB/s" \
                    if name.startswith("call") else ""
                say(f"{shape:>12s} {kind:12s} {name:32s} {med[name]:9.3f} ms  (windows {min(windows[name]):.3f}..{max(windows[name]):.3f}, "
                    f"{calls[name]} calls each){extra}")
                rows.append(dict(shape=shape, kind=kind, path=name, ms_per_call=round(med[name], 4), ms_min=round(min(windows[name]), 4),
                                 ms_max=round(max(windows[name]), 4), calls_per_window=calls[name],
                                 image_gb_per_s=round(gbs, 1) if name.startswith("call") else None))
            with_copies = med["pinned upload + call + download"]
            if full:
                host_ms = (mask_s + close_s) * 1e3
                met = with_copies < host_ms / HOST_CPUS
                say(f"{'':>12s} {'':12s} host, one core ({how}): get_mask_image {mask_s:.3f} s + closing {close_s:.3f} s; / {HOST_CPUS} CPUs = "
                    f"{host_ms / HOST_CPUS:.1f} ms; device with copies {with_copies:.3f} ms = {host_ms / with_copies:.0f} x one core, "
                    f"{host_ms / HOST_CPUS / with_copies:.1f} x sixteen: condition {'met' if met else 'NOT met'}; thresholds equal {thr_equal}, "
                    f"raw mask and count equal {raw_equal}, closed mask and count equal {closed_equal} ({int(stats[4])} -> {int(stats[5])} pixels)")
            else:
                host_ms, met = mask_s * 1e3, with_copies < mask_s * 1e3 / HOST_CPUS
                say(f"{'':>12s} {'':12s} host, one core ({how}): get_mask_image alone {mask_s:.3f} s (closing not run at this size); / {HOST_CPUS} CPUs = "
                    f"{host_ms / HOST_CPUS:.1f} ms; device with copies AND closing {with_copies:.3f} ms = {host_ms / HOST_CPUS / with_copies:.1f} x sixteen: "
                    f"condition {'met' if met else 'NOT met'}; thresholds equal {thr_equal}, raw mask and count equal {raw_equal} ({int(stats[4])} -> {int(stats[5])} pixels)")
            rows.append(dict(shape=shape, kind=kind, host_mask_s=round(mask_s, 4), host_closing_s=None if not full else round(close_s, 4), host_threads=how,
                             host_ms_over_16=round(host_ms / HOST_CPUS, 3), device_with_copies_ms=round(with_copies, 4), condition_met=bool(met),
                             thresholds_equal=thr_equal, raw_equal=raw_equal, closed_equal=closed_equal, raw_count=int(stats[4]), closed_count=int(stats[5])))
            assert thr_equal and raw_equal and closed_equal is not False, (shape, kind)
            del x, dev_buf, pinned, host_out
            torch.cuda.empty_cache()
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, floor_us=round(floor_us, 2), rows=rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
