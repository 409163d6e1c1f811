"""Tiles per second of the ResNet-50 embedder on square 256 x 256 tiles and on the reference's 256 x 265 tiles
(spatial_vis/visualize.py:212-216), in ONE process and run:
    python tools/resnet_rect_rate.py [--tiles 1000] [--rounds 5] [--modes f16x3,bf16] [--square-only] [--out profiles/resnet_rect_rate.txt]
Cases per mode: `256x256` = extract_patches_u8 on 1000 tiles of 256; `256->256x265` = imgproc.resize_u8_pil(tiles, (256, 265),
"bilinear") + extract_patches_u8 on the result, what cli/visualize.py --resnet_input reference does per chunk.  Warm-up calls
first, then `rounds` timed calls per case, the cases alternating, HIP events around each call; the line shows the median and
the spread.  The last lines set the measured time ratio beside the work ratio: per-stage output pixels of a 256 x 265 tile
over those of a 256 x 256 tile (conv1 128x133 / 128x128, layer 1 64x67 / 64x64, layer 2 32x34 / 32x32, layer 3 16x17 / 16x16,
layer 4 8x9 / 8x8), weighted by each stage's multiply-adds.  --square-only runs the 256x256 cases alone (a tree that has
no rectangular entry: the parent commit, for the square rate against it).  Prints one line per case and a last JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402


def stage_macs(H, W):
    """Multiply-adds per tile of src/resnet.py's ResNet-50 at H x W, per stage (stem, layers 1-4)."""
    c = lambda s: (s + 1) // 2
    oh, ow = c(H), c(W)
    out = [oh * ow * 64 * 147]
    h, w = c(oh), c(ow)
    inpl = 64
    for li, (planes, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3))):
        macs = 0
        for b in range(blocks):
            s = 2 if (b == 0 and li > 0) else 1
            h2, w2 = (h - 1) // s + 1, (w - 1) // s + 1
            macs += h * w * inpl * planes + h2 * w2 * 9 * planes * planes + h2 * w2 * planes * planes * 4
            if b == 0:
                macs += h2 * w2 * inpl * planes * 4
            inpl, h, w = planes * 4, h2, w2
        out.append(macs)
    return out


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="f16x3,bf16")
    ap.add_argument("--square-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    g = torch.Generator().manual_seed(256)
    x = torch.randint(0, 256, (args.tiles, 256, 256, 3), dtype=torch.uint8, generator=g).cuda()
    lines, rows = [], []
    for mode in args.modes.split(","):
        torch.manual_seed(1)
        m = resnet50(pretrained=False, compute_dtype=mode).to("cuda:0").eval()
        cases = {"256x256": lambda: m.extract_patches_u8(x)}
        if not args.square_only:
            from sequoia_pub_amd.imgproc import resize_u8_pil
            cases["256->256x265"] = lambda: m.extract_patches_u8(resize_u8_pil(x, (256, 265), "bilinear"))
        for fn in cases.values():
            for _ in range(2):
                out = fn()
            torch.cuda.synchronize()
            assert out.shape == (args.tiles, 2048) and bool(torch.isfinite(out).all())
            assert getattr(m, "last_nonfinite_reruns", 0) == 0       # the mode itself ran, not its exact-fp32 rerun
        ms = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                ms[k].append(timed_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in cases:
            row = dict(mode=mode, case=k, tiles=args.tiles, ms=round(med[k], 2), ms_min=round(min(ms[k]), 2), ms_max=round(max(ms[k]), 2),
                       tiles_per_s=round(args.tiles / med[k] * 1e3, 1))
            rows.append(row)
            lines.append(f"{mode:>7s}  {k:>14s}  {args.tiles} tiles  {med[k]:9.2f} ms  (calls {row['ms_min']:.2f}..{row['ms_max']:.2f}, {args.rounds} timed)"
                         f"  {row['tiles_per_s']:9.1f} tiles/s")
            print(lines[-1], flush=True)
        if not args.square_only:
            a, b = stage_macs(256, 265), stage_macs(256, 256)
            work = sum(a) / sum(b)
            ratio = med["256->256x265"] / med["256x256"]
            rows.append(dict(mode=mode, time_ratio=round(ratio, 3), work_ratio=round(work, 3), time_over_work=round(ratio / work, 3),
                             stage_work_ratios=[round(p / q, 3) for p, q in zip(a, b)]))
            lines.append(f"{mode:>7s}  time 256x265 (resize included) / 256x256 = {ratio:.3f}x; multiply-adds {work:.3f}x "
                         f"(per stage {', '.join(f'{p / q:.3f}' for p, q in zip(a, b))}); time ratio / work ratio = {ratio / work:.2f}")
            print(lines[-1], flush=True)
        del m, cases
        torch.cuda.empty_cache()
    lines.append(json.dumps(dict(tiles=args.tiles, rounds=args.rounds, square_only=args.square_only, rows=rows)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
