"""Regenerates tests/golden/wsi/: the JPEG-tiled TIFF / BigTIFF fixtures of tests/wsi_cases.py and wsi.npz with Pillow's
decoded bytes (libjpeg-turbo for the stand-alone tile streams, libtiff for the levels of the .tif files):

    <case>.tif               the fixture (tiles encoded by Pillow, container written by wsi_cases.write_tiff)
    <case>/L<i>              uint8 [3, height, width]   level i as Pillow opens frame i of the file (channel planes: they
                                                        deflate far better than interleaved RGB)
    <case>/L<i>/tiles        uint8 [n, 3, tile, tile]   every tile's stand-alone stream (tables joined in front) as
                                                        PIL.Image.open decodes it; photometric 2 tiles are kept as stored
    pipeline.tif, pipeline/L<i>   the synthetic slide of the pipeline tests

    python tests/golden/make_wsi_golden.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import wsi_cases as wc  # noqa: E402


def encode(tile, spec, streamtype):
    kw = dict(quality=spec["quality"], subsampling=spec["subsampling"], optimize=spec["optimize"], streamtype=streamtype)
    if spec["restart"]:
        kw["restart_marker_blocks"] = spec["restart"]
    if spec["photometric"] == 2:
        kw["keep_rgb"] = True
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(tile), "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_tile(stream):
    """A stand-alone stream as Pillow decodes it.  keep_rgb streams carry an Adobe marker with transform 0: RGB as stored."""
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def build(name, spec, out):
    levels = wc.case_levels(name)
    tile = spec["tile"]
    ifds, events = [], dict(stuffed=0, zrl=0, long_codes=0)
    for i, img in enumerate(levels):
        h, w = img.shape[:2]
        tables = None if spec["optimize"] else encode(np.zeros((16, 16, 3), np.uint8), spec, 1)
        streams, decoded = [], []
        for ty in range(-(-h // tile)):
            for tx in range(-(-w // tile)):
                s = encode(wc.pad_tile(img, tx, ty, tile), spec, 0 if spec["optimize"] else 2)
                streams.append(s)
                if name != "pipeline":
                    full = wc.join_tables(tables, s)
                    decoded.append(pil_tile(full).transpose(2, 0, 1))
                    ev = {}
                    mine = wc.decode_tile(full, spec["photometric"] == 6, ev)
                    assert np.array_equal(mine, decoded[-1].transpose(1, 2, 0)), (name, i, tx, ty)
                    for key in events:
                        events[key] += ev[key]
        if decoded:
            out[f"{name}/L{i}/tiles"] = np.stack(decoded)
        desc = wc.APERIO.format(w=w, h=h, t=tile, q=spec["quality"]) if i == 0 else None
        ifds.append(wc.level_ifd(w, h, tile, streams, spec["photometric"], spec["subsampling"], tables, desc))
        if spec["stripped"] and i == 0:
            ifds.append(wc.stripped_ifd(24, 16))
    if spec["stripped"]:
        ifds.append(wc.stripped_ifd(20, 12))
    path = os.path.join(wc.GOLDEN_DIR, f"{name}.tif")
    wc.write_tiff(path, ifds, bigtiff=spec["bigtiff"])
    with Image.open(path) as im:                        # libtiff: frames in file order, the stripped ones among them
        frame = 0
        for i in range(len(levels)):
            im.seek(frame)
            got = np.asarray(im.convert("RGB"))
            assert got.shape[:2] == levels[i].shape[:2], (name, i, got.shape)
            out[f"{name}/L{i}"] = np.ascontiguousarray(got.transpose(2, 0, 1))
            frame += 2 if (spec["stripped"] and i == 0) else 1
    if spec["content"] == "noise":                      # the case exists for these events: it must not stop covering them
        assert events["stuffed"] > 0 and events["zrl"] > 0 and events["long_codes"] > 0, events
    print(f"{name}: {os.path.getsize(path)} bytes, events {events}")


def main():
    os.makedirs(wc.GOLDEN_DIR, exist_ok=True)
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, spec in wc.CASES.items():
        build(name, spec, out)
    build("pipeline", wc.PIPELINE, out)
    np.savez_compressed(os.path.join(wc.GOLDEN_DIR, "wsi.npz"), **out)
    print("wsi.npz:", os.path.getsize(os.path.join(wc.GOLDEN_DIR, "wsi.npz")), "bytes")


if __name__ == "__main__":
    main()
