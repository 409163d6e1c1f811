"""What reading regions of an LZW or uncompressed tiled TIFF costs on the device, stage by stage, with the wave and the lane
mode of the LZW decoder alternating, beside Pillow (libtiff) decoding the same tile streams on one core, in ONE process and run
(the pattern of tools/j2k_read_rate.py):
    python tools/tiff_lzw_rate.py [--rounds 5] [--out profiles/tiff_lzw_rate.txt]
Slides, made at run time in a temporary directory: 8192 x 8192 pixels, tiles of 256, tissue-like content (flat glass around a
textured, noisy tissue region); LZW with Predictor 1, LZW with Predictor 2 (tile streams written by Pillow's libtiff), and
uncompressed.  Batches of 256 and 2048 regions of 256 x 256 pixels at seeded random level-0 corners; a batch decodes every tile
it touches once.
Per shape, after a warm-up call in each mode: `read_regions` whole (host clock around the call, which ends in the status
download) in rounds that alternate over the modes and the shapes, median and spread, and the ratio wave / lane per round; then
the stages alone -- the upload of the batch's pinned buffer (HIP events around the copy), the decode, unpredict / planes and
compose kernels (the library's event timing, rounds of their own) and the Python planning.
Host figure: PIL.Image.open(...).load() of a sample of the batch's distinct tile streams, each as a one-strip TIFF, on one
thread in the same run, scaled to the batch's tiles.  Yardstick: the device path, copies included, earns its place where its
time per batch is below the host's / 16 (a box that allows 16 CPUs can run 16 decoders side by side).
Verdict: the wave mode stays the default only if, for every LZW shape, its slowest round is below the lane mode's fastest.
Prints one line per figure and a last JSON line; --out also writes them to a file."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
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
TILE = 256
BATCHES = (256, 2048)
REGION = 256
KINDS = {"lzw_p1": (5, 1), "lzw_p2": (5, 2), "raw": (1, 1)}
MODES = {"wave": _lib._C["SQ_LZW_MODE_WAVE"], "lane": _lib._C["SQ_LZW_MODE_LANE"]}


def tissue_image(seed):
    """Tissue-like: a flat glass background around an elliptic region of low-frequency colour, texture and sensor-like noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:SIDE, 0:SIDE].astype(np.float32)
    base = np.stack([200 + 30 * np.sin(x / 310.0) * np.cos(y / 270.0), 120 + 40 * np.cos((x + y) / 420.0), 170 + 30 * np.sin(y / 150.0 - x / 510.0)], -1)
    texture = 14 * np.sin(x / 7.0 + 3 * np.sin(y / 23.0)) * np.cos(y / 5.0)
    img = np.clip(base + texture[..., None] + rng.normal(0, 3, size=(SIDE, SIDE, 1)).astype(np.float32), 0, 255).astype(np.uint8)
    inside = ((x - SIDE * 0.48) / (SIDE * 0.40)) ** 2 + ((y - SIDE * 0.52) / (SIDE * 0.36)) ** 2 < 1.0
    img[~inside] = (236, 236, 236)
    return img


def make(directory):
    from PIL import Image
    import tiffz_cases as tz
    import wsi_cases as wc
    img = tissue_image(5)
    n = SIDE // TILE
    tiles = [np.ascontiguousarray(img[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]) for ty in range(n) for tx in range(n)]
    strip = os.path.join(directory, "strip.tif")

    def libtiff_lzw(tile, predictor):
        Image.fromarray(tile).save(strip, compression="tiff_lzw", tiffinfo={278: TILE, 317: predictor})
        fd = os.open(strip, os.O_RDONLY)
        try:
            ifds, _ = wsi.read_ifds(fd, os.fstat(fd).st_size)
            return os.pread(fd, int(ifds[0][279][0]), int(ifds[0][273][0]))
        finally:
            os.close(fd)
    for kind, (compression, predictor) in KINDS.items():
        streams = [t.tobytes() if compression == 1 else libtiff_lzw(t, predictor) for t in tiles]
        path = os.path.join(directory, f"rate_{kind}.tif")
        wc.write_tiff(path, [tz.level_ifd(SIDE, SIDE, TILE, streams, compression, predictor)], bigtiff=True)
        print(f"{path}: {os.path.getsize(path) / 1e6:.1f} MB, {len(streams)} tiles", flush=True)


def spread(values):
    return statistics.median(values), min(values), max(values)


def measure(slides_dir, rounds, lines):
    import tiffz_cases as tz
    from PIL import Image
    _lib.require_gpu()
    torch.set_num_threads(1)
    host = tz.has_libtiff()
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"LZW / uncompressed TIFF read rate: {torch.cuda.get_device_name(0)}, slides of {SIDE} x {SIDE}, tiles of {TILE}, tissue-like content; "
        f"rounds {rounds}; host figure: {'Pillow (libtiff) on one thread' if host else 'no host figure (Pillow without libtiff)'}")
    shapes = []
    for kind, (compression, predictor) in KINDS.items():
        slide = wsi.TiffSlide(os.path.join(slides_dir, f"rate_{kind}.tif"), device="cuda:0", workspace_budget=16 << 30)
        for k in BATCHES:
            rng = np.random.RandomState(k)
            corners = [(int(a), int(b)) for a, b in rng.randint(0, SIDE - REGION, size=(k, 2))]
            shapes.append(dict(kind=kind, k=k, slide=slide, corners=corners, predictor=predictor, modes=list(MODES) if compression == 5 else ["wave"],
                               whole={m: [] for m in MODES}))

    def read(s, mode):
        s["slide"].lzw_mode = MODES[mode]
        out = s["slide"].read_regions(s["corners"], 0, (REGION, REGION))
        torch.cuda.synchronize()
        return out
    reference = {}
    for s in shapes:                                       # warm-up: every shape once in each mode; the modes must agree
        outs = [read(s, m) for m in s["modes"]]
        assert all(torch.equal(outs[0], o) for o in outs[1:]), (s["kind"], s["k"])
        reference.setdefault(s["k"], outs[0])
        assert torch.equal(reference[s["k"]], outs[0]), (s["kind"], s["k"])     # the three files hold the same pixels
        s["n_tiles"] = len(s["slide"].last_batch_tiles)
    del reference, outs
    for _ in range(rounds):                                # whole calls, alternating over the modes and the shapes
        for s in shapes:
            for m in s["modes"]:
                t0 = time.perf_counter()
                out = read(s, m)
                s["whole"][m].append((time.perf_counter() - t0) * 1e3)
                del out
    results = []
    for s in shapes:                                       # stages alone: kernels by the library's events, rounds of their own
        stage = {}
        for m in s["modes"]:
            _lib.prof_enable(True)
            for _ in range(rounds):
                read(s, m)
            rep = _lib.prof_report()
            _lib.prof_enable(False)
            stage[m] = {name: sum(r["total_ms"] for r in rep if r["name"].startswith(prefix)) / rounds
                        for name, prefix in (("decode", "lzw_wave" if m == "wave" and s["kind"] != "raw" else "lzw_lane"), ("unpredict", "lzw_planes"),
                                             ("compose", "jpeg_compose"))}
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
        upload = statistics.median(ups[1:])
        del pinned, dev
        host_ms = None
        if host:
            offsets, counts = s["slide"].tile_ranges(0)
            sample = tiles[::max(1, len(tiles) // 48)]      # the batch's tiles, about 48 of them timed and scaled
            files = [tz.strip_tiff(os.pread(s["slide"]._fd, int(counts[t]), int(offsets[t])), TILE, TILE, lv.codec.compression, s["predictor"]) for t in sample]
            Image.open(io.BytesIO(files[0])).load()
            t0 = time.perf_counter()
            for f in files:
                Image.open(io.BytesIO(f)).load()
            host_ms = (time.perf_counter() - t0) * 1e3 * len(tiles) / len(sample)
        row = dict(kind=s["kind"], region=REGION, regions=s["k"], tiles_decoded=len(tiles), upload_bytes=job_bytes, upload_ms=upload, python_plan_ms=plan_ms,
                   host_pillow_ms=host_ms)
        for m in s["modes"]:
            med, lo, hi = spread(s["whole"][m])
            device_ms = sum(stage[m].values()) + upload
            met = None if host_ms is None else bool(med < host_ms / HOST_CPUS)
            row[m] = dict(whole_ms=med, whole_min_ms=lo, whole_max_ms=hi, **{f"{n}_ms": v for n, v in stage[m].items()}, host_plan_read_ms=med - device_ms,
                          yardstick_met=met)
            say(f"{s['kind']:6s}  batch {s['k']:5d}  tiles decoded {len(tiles):4d}  mode {m if s['kind'] != 'raw' else '-':4s} | whole {med:9.2f} ms "
                f"({lo:.2f}..{hi:.2f}) = {med * 1e3 / s['k']:8.1f} us / region | upload {upload:7.3f}  decode {stage[m]['decode']:9.3f}  "
                f"unpredict {stage[m]['unpredict']:7.3f}  compose {stage[m]['compose']:7.3f}  Python planning {plan_ms:7.2f}  "
                f"host plan + read {med - device_ms:9.2f} ms | decode {stage[m]['decode'] * 1e3 / len(tiles):7.1f} us / tile | "
                + (f"Pillow one core {host_ms:9.1f} ms ({host_ms / len(tiles):.2f} ms / tile), / {HOST_CPUS} = {host_ms / HOST_CPUS:8.1f} ms: "
                   f"yardstick {'met' if met else 'NOT met'}" if host_ms is not None else "no host figure"))
        if len(s["modes"]) == 2:
            ratios = [w / l for w, l in zip(s["whole"]["wave"], s["whole"]["lane"])]
            med, lo, hi = spread(ratios)
            row["wave_over_lane"] = dict(median=med, min=lo, max=hi, decode_kernels=stage["wave"]["decode"] / stage["lane"]["decode"],
                                         wave_slowest_below_lane_fastest=bool(max(s["whole"]["wave"]) < min(s["whole"]["lane"])))
            say(f"{s['kind']:6s}  batch {s['k']:5d}  wave / lane: whole call {med:.3f} ({lo:.3f}..{hi:.3f} over the rounds), decode kernels alone "
                f"{row['wave_over_lane']['decode_kernels']:.3f}; the wave mode's slowest round is "
                f"{'below' if row['wave_over_lane']['wave_slowest_below_lane_fastest'] else 'NOT below'} the lane mode's fastest")
        results.append(row)
    keep = all(r["wave_over_lane"]["wave_slowest_below_lane_fastest"] for r in results if "wave_over_lane" in r)
    say(f"verdict: the wave mode {'stays' if keep else 'does NOT stay'} the default (its slowest round below the lane mode's fastest for every LZW shape: "
        f"{keep})")
    return results, keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        make(tmp)
        results, keep = measure(tmp, args.rounds, lines)
    lines.append(json.dumps(dict(tiff_lzw_rate=results, wave_stays_default=keep)))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
