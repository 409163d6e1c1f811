"""Time of the Pillow-exact device resize (imgproc.resize_u8_pil, csrc/resize.hip) beside the float path it can replace
(uni.resize_u8: fp32 copy, permute, antialiased bilinear interpolate, round, permute back), in ONE process and run:
    python tools/resize_rate.py [--patches 1000] [--seconds 1.0] [--rounds 3] [--out profiles/resize_rate.txt]
Cases: 1000 x 256 -> 224 bilinear (compute_features on the default 256-px patches) and 1000 x 512 -> 256 bicubic (the 40x
shrink of patch_gen_hdf5.py:117; uni.resize_u8 has no bicubic form, so its column there is its bilinear resize of the same
shapes).  Per case and path: warm-up calls, then `rounds` windows of about `seconds` each, the two paths alternating, every
window timed with HIP events around the whole loop of calls; the line shows the median window and the spread.  GB/s counts
one read of the uint8 input and one write of the uint8 output (the bytes the exact path needs) against the achievable HBM
rate of the MI355X, 6.3 TB/s (8 TB/s peak).  Both outputs are compared on the way: the share of bytes in which the float
path differs from the exact one.  Prints one line per case and path and a last JSON line; --out also writes them to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.imgproc import resize_u8_pil  # noqa: E402
from sequoia_pub_amd.uni import resize_u8  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0
CASES = [(256, 224, "bilinear"), (512, 256, "bicubic")]


def window_ms(fn, calls):
    """ms per call over `calls` back-to-back calls, HIP events around the loop."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of one timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows = [], []
    for size_in, size_out, resample in CASES:
        g = torch.Generator().manual_seed(size_in)
        x = torch.randint(0, 256, (args.patches, size_in, size_in, 3), dtype=torch.uint8, generator=g).cuda()
        paths = {"resize_u8_pil (" + resample + ")": lambda: resize_u8_pil(x, size_out, resample),
                 "uni.resize_u8 (float, bilinear)": lambda: resize_u8(x, size_out)}
        outs, calls, windows = {}, {}, {k: [] for k in paths}
        for name, fn in paths.items():
            for _ in range(3):
                outs[name] = fn()
            torch.cuda.synchronize()
            calls[name] = max(5, int(args.seconds * 1e3 / window_ms(fn, 5)))
        for _ in range(args.rounds):
            for name, fn in paths.items():
                windows[name].append(window_ms(fn, calls[name]))
        a, b = outs.values()
        differ = float((a != b).float().mean())
        gbytes = args.patches * 3 * (size_in * size_in + size_out * size_out) / 1e9
        for name in paths:
            ms = statistics.median(windows[name])
            row = dict(case=f"{args.patches} x {size_in} -> {size_out}", path=name, ms=round(ms, 4), ms_min=round(min(windows[name]), 4),
                       ms_max=round(max(windows[name]), 4), calls_per_window=calls[name], gb_per_call=round(gbytes, 4),
                       gbs=round(gbytes / ms * 1e3, 1), share_of_hbm=round(gbytes / ms * 1e3 / HBM_ACHIEVABLE_GBS, 3))
            rows.append(row)
            lines.append(f"{row['case']:>18s}  {name:32s} {ms:8.4f} ms  (windows {row['ms_min']:.4f}..{row['ms_max']:.4f}, {calls[name]} calls each)"
                         f"  {row['gbs']:8.1f} GB/s = {100 * row['share_of_hbm']:.1f} % of {HBM_ACHIEVABLE_GBS / 1e3:.1f} TB/s")
            print(lines[-1], flush=True)
        fast, slow = (statistics.median(windows[k]) for k in paths)
        lines.append(f"{'':>18s}  float path / exact path = {slow / fast:.2f}x; the float path's bytes differ from the exact ones in {100 * differ:.1f} %")
        print(lines[-1], flush=True)
        rows.append(dict(case=f"{args.patches} x {size_in} -> {size_out}", float_over_exact=round(slow / fast, 3), bytes_differing=round(differ, 4)))
        del x, outs, a, b, paths
        torch.cuda.empty_cache()
    lines.append(json.dumps(dict(patches=args.patches, seconds=args.seconds, rounds=args.rounds, rows=rows)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
