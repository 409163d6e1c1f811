"""What the RGBA route and the fused region -> cluster-feature path cost beside what they replace, in ONE process and run:
    python tools/region_path_rate.py [--seconds 0.5] [--rounds 3] [--tiles 2000] [--parent-lib PATH] [--out profiles/region_path_rate.txt]
(a) host time per region to fill the pinned upload buffer from an RGBA region as OpenSlide returns it: the strided
    ``[:, :, :3]`` repack (what the device path did per region) against the contiguous RGBA copy, 256 x 256 and 512 x 512
    regions, and once for a level image of 3072 x 4096 pixels (the middle size of tools/slide_mask_rate.py).  One core,
    windows of about `seconds`, the two fills alternating; median and spread.
(b) device time of the filter (1024 tiles of 256, 256 tiles of 512; with the upload from pinned memory) and of the slide
    mask (3072 x 4096, tissue-like) with pixel_bytes 3 and 4, HIP events around alternating windows.  --parent-lib: another
    build of libsequoia_hip.so (the parent commit's) whose 3-byte entries are called on the same buffers in the same
    windows, so that the existing path is timed beside what it was.
(c) tiles per second from the regions of a synthetic in-memory RGBA slide (about `tiles` kept tiles of 256 pixels) to the
    written ``cluster_features``: the three-step chain (extract_patches(device=...) -> patch file -> features file ->
    k-Means) against patchgen.embed_slide + one file, ResNet-50 f16x3 with seeded random weights, 100 clusters, with the
    bytes each path leaves on disk.  Both paths read the same regions through the same Python slide object, whose copies
    are part of both times.
The yardstick for (a) + (b): a box that allows 16 CPUs can run 16 host filters side by side, so the device path earns its
place where fill + upload + filter per tile is below the host filter's per-tile time / 16.  Prints one line per figure and
a last JSON line; --out also writes them to a file."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib, features, patchgen, store  # noqa: E402
from sequoia_pub_amd.resnet import resnet50  # noqa: E402

from patch_filter_rate import HOST_CPUS, host_keep, one_thread, tile, window_ms  # noqa: E402
from slide_mask_rate import level_image  # noqa: E402


def spread(values, scale=1.0):
    return statistics.median(values) * scale, min(values) * scale, max(values) * scale


def host_windows(fns, seconds, rounds):
    """{name: [seconds per call]}: the functions in alternating windows of about `seconds` each on this thread."""
    calls = {}
    for name, fn in fns.items():
        fn()
        t0 = time.perf_counter()
        fn()
        calls[name] = max(2, int(seconds / max(time.perf_counter() - t0, 1e-6)))
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                fn()
            out[name].append((time.perf_counter() - t0) / calls[name])
    return out


def device_windows(fns, seconds, rounds):
    calls = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(seconds * 1e3 / window_ms(fn, 3)))
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(window_ms(fn, calls[name]))
    return out


class SyntheticSlide:
    """An RGBA slide of g x g tiles of 256 pixels made of a few distinct tiles (tissue-like: kept; blank: dropped by the
    filter), with a 16 x smaller level for the mask.  read_region copies like patchgen.ArraySlide and adds alpha 255."""

    def __init__(self, g):
        kinds = np.random.RandomState(3).rand(g, g) < 0.9
        pool = {True: [tile(256, 0, 900 + i) for i in range(8)], False: [tile(256, 1, 950 + i) for i in range(4)]}
        rows = [np.concatenate([pool[bool(kinds[y, x])][(3 * y + x) % len(pool[bool(kinds[y, x])])] for x in range(g)], axis=1) for y in range(g)]
        level0 = np.concatenate(rows, axis=0)
        # the mask level: tissue colour where the tile is tissue-like, so that every such tile is a candidate
        small = np.where(np.repeat(np.repeat(kinds, 16, 0), 16, 1)[:, :, None], np.array([190, 110, 160], dtype=np.uint8), np.uint8(242))
        small = np.clip(small.astype(np.int16) + np.random.RandomState(4).randint(-6, 7, small.shape), 0, 255).astype(np.uint8)
        self.inner = patchgen.ArraySlide([level0, small])
        self.level_dimensions, self.dimensions, self.properties = self.inner.level_dimensions, self.inner.dimensions, {}

    def read_region(self, location, level, size):
        rgb = self.inner.read_region(location, level, size)
        out = np.empty(rgb.shape[:2] + (4,), dtype=np.uint8)
        out[:, :, :3] = rgb
        out[:, :, 3] = 255
        return out


def tree_bytes(root):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(root) for f in files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=2000, help="(c): about this many kept tiles")
    ap.add_argument("--parent-lib", default=None, help="another build of libsequoia_hip.so whose 3-byte entries are timed beside this one's")
    ap.add_argument("--host-tiles", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines, rows = [], []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    parent = ctypes.CDLL(args.parent_lib) if args.parent_lib else None
    stream = _lib.stream_ptr(torch.device("cuda:0"))
    limiter, how = one_thread()

    # ---- (a) + (b), tiles
    for n, size in ((1024, 256), (256, 512)):
        distinct = np.stack([tile(size, i % 3, 100 * size + i) for i in range(48)])
        regions = [np.ascontiguousarray(np.concatenate([d, np.full(d.shape[:2] + (1,), 255, np.uint8)], -1)) for d in distinct[:16]]
        pin3 = torch.empty((256, size, size, 3), dtype=torch.uint8).pin_memory()
        pin4 = torch.empty((256, size, size, 4), dtype=torch.uint8).pin_memory()
        v3, v4 = pin3.numpy(), pin4.numpy()
        state = {"k": 0}

        def fill3():
            k = state["k"] = (state["k"] + 1) % 256
            v3[k] = regions[k % 16][:, :, :3]

        def fill4():
            k = state["k"] = (state["k"] + 1) % 256
            v4[k] = regions[k % 16]

        with one_thread()[0]:
            hw = host_windows({"repack [:, :, :3]": fill3, "contiguous RGBA copy": fill4}, args.seconds, args.rounds)
        fill_us = {}
        for name, w in hw.items():
            med, lo, hi = spread(w, 1e6)
            fill_us[name] = med
            rows.append(dict(part="a", region=size, fill=name, us_per_region=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
            say(f"(a) {size} x {size} region  {name:22s} {med:9.2f} us / region  (windows {lo:.2f}..{hi:.2f}; one core, {how})")
        rgb = torch.from_numpy(distinct[np.arange(n) % 48])
        p3 = rgb.pin_memory()
        p4 = torch.cat([rgb, torch.full(rgb.shape[:3] + (1,), 255, dtype=torch.uint8)], -1).pin_memory()
        x3, x4 = p3.cuda(), p4.cuda()
        b3, b4 = torch.empty_like(x3), torch.empty_like(x4)
        keep = torch.empty(n, dtype=torch.uint8, device="cuda")
        ws_bytes = _lib.lib().sq_patch_filter_workspace_bytes(n, size, size)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        def up3():
            b3.copy_(p3, non_blocking=True)
            return patchgen.filter_patches(b3)

        def up4():
            b4.copy_(p4, non_blocking=True)
            return patchgen.filter_patches(b4)

        fns = {"filter, 3-byte pixels": lambda: patchgen.filter_patches(x3), "filter, 4-byte pixels": lambda: patchgen.filter_patches(x4),
               "upload + filter, 3-byte": up3, "upload + filter, 4-byte": up4}
        if parent is not None:
            def parent3():
                rc = parent.sq_patch_filter(_lib.ptr(x3), n, size, size, 50, ctypes.c_double(0.2), ctypes.c_double(0.05), _lib.ptr(keep), None, None,
                                            None, _lib.ptr(ws), ctypes.c_size_t(ws_bytes), stream)
                assert rc == 0
            fns["filter, 3-byte, parent build (entry alone)"] = parent3

            def ours3():
                _lib.check(_lib.lib().sq_patch_filter(_lib.ptr(x3), n, size, size, 50, 0.2, 0.05, _lib.ptr(keep), None, None, None, _lib.ptr(ws),
                                                      ws_bytes, stream))
            fns["filter, 3-byte, this build (entry alone)"] = ours3
        dw = device_windows(fns, args.seconds, args.rounds)
        assert torch.equal(patchgen.filter_patches(x3), patchgen.filter_patches(x4))
        dev_us = {}
        for name, w in dw.items():
            med, lo, hi = spread(w, 1e3 / n)
            dev_us[name] = med
            rows.append(dict(part="b", case=f"{n} x {size} x {size}", path=name, us_per_tile=round(med, 3), us_min=round(lo, 3), us_max=round(hi, 3)))
            say(f"(b) {n} x {size} x {size}  {name:44s} {med:8.3f} us / tile  (windows {lo:.3f}..{hi:.3f})")
        with one_thread()[0]:
            host_keep(distinct[0])
            t0 = time.perf_counter()
            for i in range(args.host_tiles):
                host_keep(distinct[i])
            host_us = (time.perf_counter() - t0) * 1e6 / args.host_tiles
        for label, fill, path in (("repack + 3-byte", "repack [:, :, :3]", "upload + filter, 3-byte"),
                                  ("RGBA copy + 4-byte", "contiguous RGBA copy", "upload + filter, 4-byte")):
            total = fill_us[fill] + dev_us[path]
            met = total < host_us / HOST_CPUS
            rows.append(dict(part="a+b", region=size, route=label, us_per_tile=round(total, 2), host_filter_us=round(host_us, 1),
                             host_over_16_us=round(host_us / HOST_CPUS, 1), condition_met=bool(met)))
            say(f"(a)+(b) {size} x {size}  {label:20s} fill {fill_us[fill]:.2f} + upload and filter {dev_us[path]:.2f} = {total:.2f} us / tile; host filter "
                f"{host_us / 1e3:.2f} ms / tile, / {HOST_CPUS} CPUs = {host_us / HOST_CPUS:.1f} us: with copies below host / 16 CPUs {'met' if met else 'NOT met'}")
        del x3, x4, b3, b4, p3, p4, pin3, pin4
        torch.cuda.empty_cache()

    # ---- (a) + (b), the level image
    H, W = 3072, 4096
    img = level_image(H, W, "tissue-like", 1)
    img4 = np.ascontiguousarray(np.concatenate([img, np.full((H, W, 1), 255, np.uint8)], -1))
    pin3 = torch.empty((H, W, 3), dtype=torch.uint8).pin_memory()
    pin4 = torch.empty((H, W, 4), dtype=torch.uint8).pin_memory()
    v3, v4 = pin3.numpy(), pin4.numpy()

    def level3():
        v3[...] = img4[:, :, :3]

    def level4():
        v4[...] = img4

    with one_thread()[0]:
        hw = host_windows({"repack [:, :, :3]": level3, "contiguous RGBA copy": level4}, args.seconds, args.rounds)
    for name, w in hw.items():
        med, lo, hi = spread(w, 1e3)
        rows.append(dict(part="a", level=f"{H} x {W}", fill=name, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3)))
        say(f"(a) {H} x {W} level image  {name:22s} {med:9.3f} ms  (windows {lo:.3f}..{hi:.3f}; one core)")
    x3, x4 = pin3.cuda(), pin4.cuda()
    fns = {"slide mask, 3-byte pixels": lambda: patchgen.slide_mask(x3, transpose=True), "slide mask, 4-byte pixels": lambda: patchgen.slide_mask(x4, transpose=True)}
    if parent is not None:
        closed = torch.empty((W, H), dtype=torch.uint8, device="cuda")
        ws_bytes = _lib.lib().sq_slide_mask_workspace_bytes(H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        def parent_mask():
            assert parent.sq_slide_mask(_lib.ptr(x3), H, W, 50, 3, 1, None, _lib.ptr(closed), None, _lib.ptr(ws), ctypes.c_size_t(ws_bytes), stream) == 0

        def our_mask():
            _lib.check(_lib.lib().sq_slide_mask(_lib.ptr(x3), H, W, 50, 3, 1, None, _lib.ptr(closed), None, _lib.ptr(ws), ws_bytes, stream))
        fns["slide mask, 3-byte, parent build (entry alone)"] = parent_mask
        fns["slide mask, 3-byte, this build (entry alone)"] = our_mask
    dw = device_windows(fns, args.seconds, args.rounds)
    assert torch.equal(patchgen.slide_mask(x3, transpose=True), patchgen.slide_mask(x4, transpose=True))
    for name, w in dw.items():
        med, lo, hi = spread(w)
        rows.append(dict(part="b", case=f"{H} x {W}", path=name, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4)))
        say(f"(b) {H} x {W}  {name:48s} {med:8.4f} ms  (windows {lo:.4f}..{hi:.4f})")
    del x3, x4, pin3, pin4, img, img4
    torch.cuda.empty_cache()

    # ---- (c) regions -> cluster_features
    g = int(np.ceil(np.sqrt(args.tiles / 0.9))) + 1                 # the closing clears the mask's frame: one row and column more
    slide = SyntheticSlide(g)
    torch.manual_seed(1)
    model = resnet50(pretrained=False, compute_dtype="f16x3").to("cuda:0").eval()
    root = tempfile.mkdtemp(prefix="region_path_")

    def chain(d):
        patchgen.extract_patches(slide, os.path.join(d, "masks"), (256, 256), os.path.join(d, "patches"), "S", None, device="cuda:0",
                                 slide_mask="device")
        with store.File(os.path.join(d, "patches", "S", "S.hdf5"), "r") as f:
            keys = features.sample_keys(f.keys(), 4000)
            patches = torch.from_numpy(np.stack([np.asarray(f[k][:]) for k in keys]))
        feats = features.patch_features(model, patches, "resnet", "float", "cuda:0").cpu().numpy()
        os.makedirs(os.path.join(d, "features"))
        with store.File(os.path.join(d, "features", "S.h5"), "w") as f:
            f.create_dataset("resnet_features", data=feats)
        with store.File(os.path.join(d, "features", "S.h5"), "r+") as f:
            x = np.asarray(f["resnet_features"][:])
            f.create_dataset("cluster_features", data=features.cluster(torch.from_numpy(x).to("cuda:0"), 100)["cluster_features"][0].cpu().numpy())
        return len(keys)

    def fused(d):
        r = patchgen.embed_slide(slide, model, patch_size=(256, 256), max_patches_per_slide=None, max_patch_number=4000, n_clusters=100,
                                 feat_type="resnet", resize="float", device="cuda:0", slide_mask="device", mask_path=os.path.join(d, "masks"),
                                 slide_id="S")
        os.makedirs(os.path.join(d, "features"))
        with store.File(os.path.join(d, "features", "S.h5"), "w") as f:
            f.create_dataset("resnet_features", data=r["features"].cpu().numpy())
            f.create_dataset("coords", data=r["coords"])
            f.create_dataset("cluster_features", data=r["cluster_features"].cpu().numpy())
        return int(r["coords"].shape[0])

    times, kept, disk = {"chain": [], "fused": []}, {}, {}
    try:
        for rnd in range(args.rounds + 1):                          # round 0 warms both paths up
            for name, fn in (("chain", chain), ("fused", fused)):
                d = os.path.join(root, f"{name}{rnd}")
                os.makedirs(d)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with open(os.devnull, "w") as null, _quiet(null):
                    kept[name] = fn(d)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t0)
                disk[name] = tree_bytes(d)
                shutil.rmtree(d)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    assert kept["chain"] == kept["fused"]
    for name in ("chain", "fused"):
        med, lo, hi = spread(times[name])
        rows.append(dict(part="c", path=name, kept_tiles=kept[name], seconds=round(med, 3), s_min=round(lo, 3), s_max=round(hi, 3),
                         tiles_per_s=round(kept[name] / med, 1), bytes_on_disk=disk[name]))
        say(f"(c) {g} x {g} tiles, {kept[name]} kept  {name:6s} {med:7.3f} s  (runs {lo:.3f}..{hi:.3f})  {kept[name] / med:8.1f} tiles / s  "
            f"{disk[name] / 1e6:9.1f} MB written")
    say(json.dumps(dict(seconds=args.seconds, rounds=args.rounds, parent_lib=bool(parent), rows=rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


class _quiet:
    """The per-slide prints of the two paths go nowhere while they are timed."""

    def __init__(self, sink):
        self.sink = sink

    def __enter__(self):
        self.saved, sys.stdout = sys.stdout, self.sink

    def __exit__(self, *a):
        sys.stdout = self.saved


if __name__ == "__main__":
    main()
