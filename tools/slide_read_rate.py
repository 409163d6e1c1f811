"""What reading regions of a JPEG-tiled slide costs on the device, stage by stage, beside Pillow decoding the same tile
streams on one core, in ONE process and run:
    python tools/slide_read_rate.py --make DIR      # needs Pillow with JPEG: writes the synthetic slides (done where Pillow has it)
    python tools/slide_read_rate.py --slides DIR [--rounds 5] [--out profiles/slide_read_rate.txt]
Slides: 8192 x 8192 pixels, tiles of 240 and of 256 pixels, 4:2:2, quality 70, photographic-like content (smooth structure
plus noise), one JPEGTables stream.  Batches of 256, 2048 and 16384 regions of 256 x 256 and of 512 x 512 pixels at seeded
random level-0 corners; a batch decodes every tile it touches once, so the figures are given per region AND per decoded tile
(the large batches touch every tile of the slide and mostly compose).
Per shape, after a warm-up call: `read_regions` whole (host clock around the call, which ends in the status download) in
rounds that alternate over the shapes, median and spread; then the stages alone -- the upload of the batch's pinned buffer
(HIP events around the copy), and the entropy, IDCT and compose kernels (the library's event timing, rounds of their own).
What is left of the whole is the host's planning and file reads.
Host figure: PIL.Image.open(...).convert("RGB") of the batch's distinct tile streams (tables joined in front) on one thread
in the same run; "no host figure" where Pillow has no JPEG.  Yardstick: the device path, copies included, earns its place
where its time per batch is below the host's / 16 (a box that allows 16 CPUs can run 16 decoders side by side).
Prints one line per figure and a last JSON line; --out also writes them to a file."""
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

HOST_CPUS = 16
SIDE = 8192
TILES = (240, 256)
BATCHES = (256, 2048, 16384)
REGIONS = (256, 512)


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


def measure(slides_dir, rounds, lines):
    _lib.require_gpu()
    torch.set_num_threads(1)
    decode = pillow_decoder()
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"slide read rate: {torch.cuda.get_device_name(0)}, slides of {SIDE} x {SIDE}, 4:2:2, quality 70; rounds {rounds}; "
        f"host figure: {'Pillow on one thread' if decode else 'no host figure (Pillow without JPEG)'}")
    results = []
    shapes = []
    for tile in TILES:
        slide = wsi.TiffSlide(os.path.join(slides_dir, f"rate_{tile}.tif"), device="cuda:0", workspace_budget=8 << 30)
        for size in REGIONS:
            for k in BATCHES:
                rng = np.random.RandomState(k + size + tile)
                corners = [(int(a), int(b)) for a, b in rng.randint(0, SIDE - size, size=(k, 2))]
                shapes.append(dict(tile=tile, size=size, k=k, slide=slide, corners=corners, whole=[]))
    for s in shapes:                                       # warm-up: every shape once, and what it decodes
        s["slide"].read_regions(s["corners"], 0, (s["size"], s["size"]))
        s["n_tiles"] = len(s["slide"].last_batch_tiles)
        torch.cuda.synchronize()
    for _ in range(rounds):                                # whole calls, alternating over the shapes
        for s in shapes:
            t0 = time.perf_counter()
            out = s["slide"].read_regions(s["corners"], 0, (s["size"], s["size"]))
            torch.cuda.synchronize()
            s["whole"].append((time.perf_counter() - t0) * 1e3)
            del out
    for s in shapes:                                       # stages alone: kernels by the library's events, rounds of their own
        _lib.prof_enable(True)
        for _ in range(rounds):
            s["slide"].read_regions(s["corners"], 0, (s["size"], s["size"]))
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        stage = {"entropy": 0.0, "idct": 0.0, "compose": 0.0, "tables": 0.0}
        for r in rep:
            for name in stage:
                if r["name"].startswith(f"jpeg_{name}"):
                    stage[name] += r["total_ms"] / rounds
        lv = s["slide"]._levels[0]
        tiles = sorted({ty * lv.tiles_x + tx for tx, ty in s["slide"].last_batch_tiles})
        job_bytes = int(sum(s["slide"]._tile_info(lv, t)[1] for t in tiles)) + len(tiles) * 32 + lv.tiles_x * lv.tiles_y * 4 + s["k"] * 8
        pinned = torch.empty(job_bytes, dtype=torch.uint8).pin_memory()
        ups = []
        for _ in range(rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev = pinned.to("cuda:0", non_blocking=True)
            b.record()
            b.synchronize()
            ups.append(a.elapsed_time(b))
        stage["upload"] = statistics.median(ups[1:])
        host_ms = None
        if decode:
            offsets, counts = s["slide"].tile_ranges(0)
            ifds, _ = wsi.read_ifds(s["slide"]._fd, s["slide"]._size)
            tables = bytes(ifds[lv.index][347])
            sample = tiles[::max(1, len(tiles) // 256)]     # the batch's tiles, at most ~256 of them timed and scaled
            streams = [tables[:-2] + os.pread(s["slide"]._fd, int(counts[t]), int(offsets[t]))[2:] for t in sample]
            decode(streams[0])
            t0 = time.perf_counter()
            for st in streams:
                decode(st)
            host_ms = (time.perf_counter() - t0) * 1e3 * len(tiles) / len(sample)
        med, lo, hi = spread(s["whole"])
        device_ms = sum(stage.values())
        met = None if host_ms is None else bool(med < host_ms / HOST_CPUS)
        row = dict(tile=s["tile"], region=s["size"], regions=s["k"], tiles_decoded=len(tiles), upload_bytes=job_bytes, whole_ms=med,
                   whole_min_ms=lo, whole_max_ms=hi, **{f"{n}_ms": v for n, v in stage.items()}, host_plan_read_ms=med - device_ms,
                   host_pillow_ms=host_ms, yardstick_met=met)
        results.append(row)
        say(f"tile {s['tile']:3d}  region {s['size']:3d}  batch {s['k']:5d}  tiles decoded {len(tiles):4d} | whole {med:9.2f} ms ({lo:.2f}..{hi:.2f}) = "
            f"{med * 1e3 / s['k']:8.1f} us / region | upload {stage['upload']:7.3f}  entropy {stage['entropy']:8.3f}  idct {stage['idct']:7.3f}  "
            f"compose {stage['compose']:8.3f}  host plan + read {med - device_ms:9.2f} ms | entropy {stage['entropy'] * 1e3 / len(tiles):7.1f} us / tile | "
            + (f"Pillow one core {host_ms:9.1f} ms, / {HOST_CPUS} = {host_ms / HOST_CPUS:8.1f} ms: yardstick {'met' if met else 'NOT met'}"
               if host_ms is not None else "no host figure"))
    return results


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
    results = measure(args.slides, args.rounds, lines)
    lines.append(json.dumps(dict(slide_read_rate=results)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
