"""What reading regions of a JPEG 2000 SVS slide costs on the device, stage by stage, beside Pillow (OpenJPEG) decoding the
same tile streams on one core, in ONE process and run (the pattern of tools/slide_read_rate.py):
    python tools/j2k_read_rate.py --make DIR      # needs Pillow with JPEG 2000: writes the synthetic slides
    python tools/j2k_read_rate.py --slides DIR [--rounds 3] [--out profiles/j2k_read_rate.txt]
Slides: 8192 x 8192 pixels, tiles of 240 pixels, lossy 9/7 at 38 dB, 5 levels, 64 x 64 code-blocks, one layer; one with
compression 33005 and the irreversible component transform, one with 33003 as 4:2:2 without it (tests/j2k_cases.py's
construction); the photographic-like content of tools/slide_read_rate.py.  Batches of 256, 2048 and 16384 regions of 256 x 256
and of 512 x 512 pixels at seeded random level-0 corners; a batch decodes every tile it touches once.
Per shape, after a warm-up call: `read_regions` whole (host clock around the call, which ends in the status download) in
rounds that alternate over the shapes, median and spread; then the stages alone -- the upload of the batch's pinned buffer
(HIP events around the copy) and the packet, code-block, wavelet, plane and compose kernels (the library's event timing,
rounds of their own).  What is left of the whole is the host's planning and file reads.
Host figure: PIL.Image.open(...).load() of a sample of the batch's distinct tile streams on one thread in the same run, scaled
to the batch's tiles.  Yardstick: the device path, copies included, earns its place where its time per batch is below the
host's / 16 (a box that allows 16 CPUs can run 16 decoders side by side).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, wsi  # noqa: E402

HOST_CPUS = 16
SIDE = 8192
TILE = 240
BATCHES = (256, 2048, 16384)
REGIONS = (256, 512)
KINDS = {"33005_ict": dict(compression=33005, opts=dict(irreversible=True, quality_mode="dB", quality_layers=[38], num_resolutions=6, mct=1, codeblock_size=(64, 64))),
         "33003_422": dict(compression=33003, s422=True, opts=dict(irreversible=True, quality_mode="dB", quality_layers=[38], num_resolutions=6, codeblock_size=(64, 64)))}
STAGES = ("packets", "blocks", "idwt", "planes")


def make(directory):
    import j2k_cases as jc
    import wsi_cases as wc
    from slide_read_rate import slide_image
    os.makedirs(directory, exist_ok=True)
    img = slide_image(5)
    n = -(-SIDE // TILE)
    for kind, spec in KINDS.items():
        streams = [jc.encode_tile(jc.pad_tile(img, tx, ty, (TILE, TILE)), spec)[0] for ty in range(n) for tx in range(n)]
        path = os.path.join(directory, f"rate_{kind}.tif")
        wc.write_tiff(path, [wc.level_ifd(SIDE, SIDE, TILE, streams, 6 if spec["compression"] == 33003 else 2, 1 if spec.get("s422") else 0, None,
                                          jc.APERIO.format(w=SIDE, h=SIDE, tw=TILE, th=TILE), compression=spec["compression"])], bigtiff=True)
        print(f"{path}: {os.path.getsize(path) / 1e6:.1f} MB, {len(streams)} tiles", flush=True)


def spread(values):
    return statistics.median(values), min(values), max(values)


def pillow_decoder():
    try:
        from PIL import Image, features
        if features.check_codec("jpg_2000"):
            return lambda s: Image.open(io.BytesIO(s)).load()
    except ImportError:
        pass
    return None


def measure(slides_dir, rounds, lines):
    _lib.require_gpu()
    torch.set_num_threads(1)
    decode = pillow_decoder()
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"JPEG 2000 slide read rate: {torch.cuda.get_device_name(0)}, slides of {SIDE} x {SIDE}, tiles of {TILE}, 9/7 at 38 dB; rounds {rounds}; "
        f"host figure: {'Pillow (OpenJPEG) on one thread' if decode else 'no host figure (Pillow without JPEG 2000)'}")
    shapes = []
    for kind in KINDS:
        slide = wsi.TiffSlide(os.path.join(slides_dir, f"rate_{kind}.tif"), device="cuda:0", workspace_budget=16 << 30)
        for size in REGIONS:
            for k in BATCHES:
                rng = np.random.RandomState(k + size)
                corners = [(int(a), int(b)) for a, b in rng.randint(0, SIDE - size, size=(k, 2))]
                shapes.append(dict(kind=kind, size=size, k=k, slide=slide, corners=corners, whole=[]))
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
    results = []
    for s in shapes:                                       # stages alone: kernels by the library's events, rounds of their own
        _lib.prof_enable(True)
        for _ in range(rounds):
            s["slide"].read_regions(s["corners"], 0, (s["size"], s["size"]))
        rep = _lib.prof_report()
        _lib.prof_enable(False)
        stage = {name: 0.0 for name in STAGES + ("compose",)}
        for r in rep:
            for name in STAGES:
                if r["name"].startswith(f"j2k_{name}"):
                    stage[name] += r["total_ms"] / rounds
            if r["name"].startswith("jpeg_compose"):
                stage["compose"] += r["total_ms"] / rounds
        lv = s["slide"]._levels[0]
        tiles = sorted({ty * lv.tiles_x + tx for tx, ty in s["slide"].last_batch_tiles})
        t0 = time.perf_counter()
        s["slide"]._plan(lv, tiles)
        plan_ms = (time.perf_counter() - t0) * 1e3
        job_bytes = int(sum(s["slide"]._tile_info(lv, t).length for t in tiles)) + len(tiles) * lv.codec.tile_words * 4 + lv.tiles_x * lv.tiles_y * 4 + s["k"] * 8
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
            sample = tiles[::max(1, len(tiles) // 48)]      # the batch's tiles, about 48 of them timed and scaled
            streams = [os.pread(s["slide"]._fd, int(counts[t]), int(offsets[t])) for t in sample]
            decode(streams[0])
            t0 = time.perf_counter()
            for st in streams:
                decode(st)
            host_ms = (time.perf_counter() - t0) * 1e3 * len(tiles) / len(sample)
        med, lo, hi = spread(s["whole"])
        device_ms = sum(stage.values())
        met = None if host_ms is None else bool(med < host_ms / HOST_CPUS)
        row = dict(kind=s["kind"], region=s["size"], regions=s["k"], tiles_decoded=len(tiles), upload_bytes=job_bytes, whole_ms=med,
                   whole_min_ms=lo, whole_max_ms=hi, **{f"{n}_ms": v for n, v in stage.items()}, python_plan_ms=plan_ms,
                   host_plan_read_ms=med - device_ms, host_pillow_ms=host_ms, yardstick_met=met)
        results.append(row)
        say(f"{s['kind']}  region {s['size']:3d}  batch {s['k']:5d}  tiles decoded {len(tiles):4d} | whole {med:9.2f} ms ({lo:.2f}..{hi:.2f}) = "
            f"{med * 1e3 / s['k']:8.1f} us / region | upload {stage['upload']:7.3f}  packets {stage['packets']:8.3f}  blocks {stage['blocks']:9.3f}  "
            f"wavelet {stage['idwt']:8.3f}  planes {stage['planes']:7.3f}  compose {stage['compose']:8.3f}  Python planning {plan_ms:7.2f}  "
            f"host plan + read {med - device_ms:9.2f} ms | blocks {stage['blocks'] * 1e3 / len(tiles):7.1f} us / tile | "
            + (f"Pillow one core {host_ms:9.1f} ms ({host_ms / len(tiles):.2f} ms / tile), / {HOST_CPUS} = {host_ms / HOST_CPUS:8.1f} ms: "
               f"yardstick {'met' if met else 'NOT met'}" if host_ms is not None else "no host figure"))
    return results


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--make", default=None)
    p.add_argument("--slides", default=None)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.make:
        make(args.make)
        return
    lines = []
    results = measure(args.slides, args.rounds, lines)
    lines.append(json.dumps(dict(j2k_read_rate=results)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
