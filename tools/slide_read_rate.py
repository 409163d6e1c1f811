"""What reading regions of a JPEG-tiled slide costs on the device, stage by stage, beside Pillow decoding the same tile
streams on one core, in ONE process and run:
    python tools/slide_read_rate.py --make DIR      # needs Pillow with JPEG: writes the synthetic slides (done where Pillow has it)
    python tools/slide_read_rate.py --slides DIR [--rounds 5] [--out profiles/slide_read_rate.txt]
Slides: 8192 x 8192 pixels, tiles of 240 and of 256 pixels, 4:2:2, quality 70, photographic-like content (smooth structure
plus noise), one JPEGTables stream.  Batches of 256, 2048 and 16384 regions of 256 x 256 and of 512 x 512 pixels at seeded
random level-0 corners; a batch decodes every tile it touches once, so the figures are given per region AND per decoded tile
(the large batches touch every tile of the slide and mostly compose).
Both entropy modes of the reader are timed in the one run, `TiffSlide(entropy="serial")` and `entropy="split"` (the library's
default sub_bytes), alternating within each shape.  Per shape and mode, after a warm-up call: `read_regions` whole (host clock
around the call, which ends in the status download) in rounds that alternate over the shapes and modes, median and spread; then
the stages alone -- the upload of the batch's pinned buffer (HIP events around the copy), and the entropy, IDCT and compose
kernels (the library's event timing, one profiled call per round and mode; the entropy stage with its min..max over the rounds).
What is left of the whole is the host's planning and file reads.  A line per shape says whether the split mode's slowest
entropy round is below the serial mode's fastest.  Last, the split mode's entropy stage over sub_bytes 32, 64, 128 and 256 on
the 256-region and 2048-region shapes.
Host figure: PIL.Image.open(...).convert("RGB") of the batch's distinct tile streams (tables joined in front) on one thread
in the same run; "no host figure" where Pillow has no JPEG.  Yardstick: the device path, copies included, earns its place
where its time per batch is below the host's / 16 (a box that allows 16 CPUs can run 16 decoders side by side).
Prints one line per figure and a last JSON line; --out also appends them to a file as a new dated section."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, wsi  # noqa: E402
from sequoia_pub_amd._abi import CONSTANTS as _C  # noqa: E402

HOST_CPUS = 16
SIDE = 8192
TILES = (240, 256)
BATCHES = (256, 2048, 16384)
REGIONS = (256, 512)
MODES = ("serial", "split")                  # TiffSlide(entropy=...): one lane per tile, or a wave per tile
SWEEP_SUBS = (32, 64, 128, 256)              # sub_bytes of the split mode, timed on the batches of SWEEP_BATCHES
SWEEP_BATCHES = (256, 2048)


def slide_image(seed):
    """Photographic-like: low-frequency colour structure, mid-frequency texture and sensor-like noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:SIDE, 0:SIDE].astype(np.float32)
    base = np.stack([170 + 50 * np.sin(x / 310.0) * np.cos(y / 270.0), 120 + 60 * np.cos((x + y) / 420.0), 160 + 40 * np.sin(y / 150.0 - x / 510.0)], -1)
    texture = 18 * np.sin(x / 7.0 + 3 * np.sin(y / 23.0)) * np.cos(y / 5.0)
    img = base + texture[..., None] + rng.normal(0, 6, size=(SIDE, SIDE, 1)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def make(directory):
    from PIL import Image
    import wsi_cases as wc
    os.makedirs(directory, exist_ok=True)
    img = slide_image(5)
    for tile in TILES:
        def enc(a, streamtype):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(a), "RGB").save(buf, "JPEG", quality=70, subsampling=1, streamtype=streamtype)
            return buf.getvalue()
        n = -(-SIDE // tile)
        streams = [enc(wc.pad_tile(img, tx, ty, tile), 2) for ty in range(n) for tx in range(n)]
        path = os.path.join(directory, f"rate_{tile}.tif")
        wc.write_tiff(path, [wc.level_ifd(SIDE, SIDE, tile, streams, 6, 1, enc(np.zeros((16, 16, 3), np.uint8), 1),
                                          wc.APERIO.format(w=SIDE, h=SIDE, t=tile, q=70))], bigtiff=True)
        print(f"{path}: {os.path.getsize(path) / 1e6:.1f} MB, {len(streams)} tiles")


def spread(values):
    return statistics.median(values), min(values), max(values)


def pillow_decoder():
    try:
        from PIL import Image, features
        if features.check("jpg"):
            return lambda s: np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))
    except ImportError:
        pass
    return None


def stages_of(report):
    stage = {"entropy": 0.0, "idct": 0.0, "compose": 0.0, "tables": 0.0}
    for r in report:
        for name in stage:
            if r["name"].startswith(f"jpeg_{name}"):
                stage[name] += r["total_ms"]
    return stage


def profiled_call(slide, corners, size):
    """One read_regions call with the library's event timing on: {stage: ms} of that call."""
    _lib.prof_enable(True)
    slide.read_regions(corners, 0, (size, size))
    rep = _lib.prof_report()
    _lib.prof_enable(False)
    return stages_of(rep)


def measure(slides_dir, rounds, lines):
    _lib.require_gpu()
    torch.set_num_threads(1)
    decode = pillow_decoder()
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"slide read rate: {torch.cuda.get_device_name(0)}, slides of {SIDE} x {SIDE}, 4:2:2, quality 70; rounds {rounds}; "
        f"entropy modes {' and '.join(MODES)} alternating within each shape (split: sub_bytes {_C['SQ_JPEG_SPLIT_SUB_DEFAULT']}, the library's default); "
        f"host figure: {'Pillow on one thread' if decode else 'no host figure (Pillow without JPEG)'}")
    results = []
    shapes = []
    for tile in TILES:
        path = os.path.join(slides_dir, f"rate_{tile}.tif")
        slides = {mode: wsi.TiffSlide(path, device="cuda:0", workspace_budget=8 << 30, entropy=mode) for mode in MODES}
        for size in REGIONS:
            for k in BATCHES:
                rng = np.random.RandomState(k + size + tile)
                corners = [(int(a), int(b)) for a, b in rng.randint(0, SIDE - size, size=(k, 2))]
                shapes.append(dict(tile=tile, size=size, k=k, slides=slides, path=path, corners=corners, whole={m: [] for m in MODES},
                                   stages={m: [] for m in MODES}))
    for s in shapes:                                       # warm-up: every shape once in each mode, and what it decodes
        for mode in MODES:
            s["slides"][mode].read_regions(s["corners"], 0, (s["size"], s["size"]))
        s["n_tiles"] = len(s["slides"]["serial"].last_batch_tiles)
        torch.cuda.synchronize()
    for _ in range(rounds):                                # whole calls, alternating over the shapes and, within a shape, the modes
        for s in shapes:
            for mode in MODES:
                t0 = time.perf_counter()
                out = s["slides"][mode].read_regions(s["corners"], 0, (s["size"], s["size"]))
                torch.cuda.synchronize()
                s["whole"][mode].append((time.perf_counter() - t0) * 1e3)
                del out
    for s in shapes:                                       # stages alone: kernels by the library's events, rounds of their own
        for _ in range(rounds):
            for mode in MODES:
                s["stages"][mode].append(profiled_call(s["slides"][mode], s["corners"], s["size"]))
        slide = s["slides"]["serial"]
        lv = slide._levels[0]
        tiles = sorted({ty * lv.tiles_x + tx for tx, ty in slide.last_batch_tiles})
        job_bytes = int(sum(slide._tile_info(lv, t).length for t in tiles)) + len(tiles) * lv.codec.tile_words * 4 + lv.tiles_x * lv.tiles_y * 4 + s["k"] * 8
        pinned = torch.empty(job_bytes, dtype=torch.uint8).pin_memory()
        ups = []
        for _ in range(rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev = pinned.to("cuda:0", non_blocking=True)
            b.record()
            b.synchronize()
            ups.append(a.elapsed_time(b))
        upload = statistics.median(ups[1:])
        host_ms = None
        if decode:
            offsets, counts = slide.tile_ranges(0)
            ifds, _ = wsi.read_ifds(slide._fd, slide._size)
            tables = bytes(ifds[lv.index][347])
            sample = tiles[::max(1, len(tiles) // 256)]     # the batch's tiles, at most ~256 of them timed and scaled
            streams = [tables[:-2] + os.pread(slide._fd, int(counts[t]), int(offsets[t]))[2:] for t in sample]
            decode(streams[0])
            t0 = time.perf_counter()
            for st in streams:
                decode(st)
            host_ms = (time.perf_counter() - t0) * 1e3 * len(tiles) / len(sample)
        rows = {}
        for mode in MODES:
            med, lo, hi = spread(s["whole"][mode])
            stage = {n: statistics.median(r[n] for r in s["stages"][mode]) for n in ("entropy", "idct", "compose", "tables")}
            _, e_lo, e_hi = spread([r["entropy"] for r in s["stages"][mode]])
            stage["upload"] = upload
            device_ms = sum(stage.values())
            met = None if host_ms is None else bool(med < host_ms / HOST_CPUS)
            rows[mode] = dict(mode=mode, tile=s["tile"], region=s["size"], regions=s["k"], tiles_decoded=len(tiles), upload_bytes=job_bytes,
                              whole_ms=med, whole_min_ms=lo, whole_max_ms=hi, **{f"{n}_ms": v for n, v in stage.items()},
                              entropy_min_ms=e_lo, entropy_max_ms=e_hi, host_plan_read_ms=med - device_ms, host_pillow_ms=host_ms, yardstick_met=met)
            results.append(rows[mode])
            say(f"tile {s['tile']:3d}  region {s['size']:3d}  batch {s['k']:5d}  {mode:6s}  tiles decoded {len(tiles):4d} | whole {med:9.2f} ms ({lo:.2f}..{hi:.2f}) = "
                f"{med * 1e3 / s['k']:8.1f} us / region | upload {stage['upload']:7.3f}  entropy {stage['entropy']:8.3f} ({e_lo:.3f}..{e_hi:.3f})  idct {stage['idct']:7.3f}  "
                f"compose {stage['compose']:8.3f}  host plan + read {med - device_ms:9.2f} ms | entropy {stage['entropy'] * 1e3 / len(tiles):7.1f} us / tile | "
                + (f"Pillow one core {host_ms:9.1f} ms, / {HOST_CPUS} = {host_ms / HOST_CPUS:8.1f} ms: yardstick {'met' if met else 'NOT met'}"
                   if host_ms is not None else "no host figure"))
        faster = rows["split"]["entropy_max_ms"] < rows["serial"]["entropy_min_ms"]      # by more than the two modes' own spread
        rows["split"]["entropy_faster_beyond_spread"] = bool(faster)
        say(f"tile {s['tile']:3d}  region {s['size']:3d}  batch {s['k']:5d}  entropy stage, split against serial: {rows['serial']['entropy_ms'] / rows['split']['entropy_ms']:.1f} x; "
            f"split's slowest round {'below' if faster else 'NOT below'} serial's fastest")
    sweep = []
    say(f"sub_bytes sweep, entropy stage of the split mode in ms (median of {rounds} rounds that alternate over the sizes):")
    for s in shapes:
        if s["k"] not in SWEEP_BATCHES:
            continue
        slides = {sub: wsi.TiffSlide(s["path"], device="cuda:0", workspace_budget=8 << 30, entropy="split", sub_bytes=sub) for sub in SWEEP_SUBS}
        for sub in SWEEP_SUBS:
            slides[sub].read_regions(s["corners"], 0, (s["size"], s["size"]))
        torch.cuda.synchronize()
        got = {sub: [] for sub in SWEEP_SUBS}
        for _ in range(rounds):
            for sub in SWEEP_SUBS:
                got[sub].append(profiled_call(slides[sub], s["corners"], s["size"])["entropy"])
        med = {sub: statistics.median(got[sub]) for sub in SWEEP_SUBS}
        sweep.append(dict(tile=s["tile"], region=s["size"], regions=s["k"], **{f"sub{sub}_ms": med[sub] for sub in SWEEP_SUBS}))
        say(f"tile {s['tile']:3d}  region {s['size']:3d}  batch {s['k']:5d} | " + "  ".join(f"sub_bytes {sub:3d}: {med[sub]:7.3f}" for sub in SWEEP_SUBS)
            + f" | fastest {min(med, key=med.get)}")
        for sl in slides.values():
            sl.close()
    return results, sweep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--make", default=None)
    p.add_argument("--slides", default=None)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.make:
        make(args.make)
        return
    lines = []
    results, sweep = measure(args.slides, args.rounds, lines)
    lines.append(json.dumps(dict(slide_read_rate=results, sub_bytes_sweep=sweep)))
    print(lines[-1])
    if args.out:                                           # a new dated section behind what the file holds
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(f"==== {time.strftime('%Y-%m-%d')}: serial and split entropy decode ====\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
