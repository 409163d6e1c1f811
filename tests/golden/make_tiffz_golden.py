"""Regenerates tests/golden/tiffz/: the LZW and uncompressed tiled-TIFF fixtures of tests/tiffz_cases.py and tiffz.npz.

    <case>.tif      the fixture: every LZW tile stream is Pillow's libtiff's (the padded tile saved as a one-strip TIFF with
                    compression 'tiff_lzw' and the case's predictor, and the strip's bytes taken), uncompressed tiles are the
                    bytes themselves; the container is written by wsi_cases.write_tiff
    <case>/L<i>     uint8 [h, w, 3]   level i as Pillow opens the finished file
    pipeline.tif, pipeline/L<i>       the synthetic slide of the pipeline tests

Every level Pillow opens is asserted equal to the image the tiles were cut from (the formats are lossless), and every case is
run through tools/lzw_hostcheck.cpp against those bytes.

    python tests/golden/make_tiffz_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import tiffz_cases as tz  # noqa: E402
import wsi_cases as wc  # noqa: E402
from sequoia_pub_amd import wsi  # noqa: E402


def libtiff_lzw(tile, predictor, tmp):
    """The LZW strip libtiff writes for a chunky uint8 tile [h, w, 3]."""
    path = os.path.join(tmp, "strip.tif")
    Image.fromarray(np.ascontiguousarray(tile)).save(path, compression="tiff_lzw", tiffinfo={278: tile.shape[0], 317: predictor})
    fd = os.open(path, os.O_RDONLY)
    try:
        ifds, _ = wsi.read_ifds(fd, os.fstat(fd).st_size)
        assert len(ifds) == 1 and len(ifds[0][273]) == 1 and int(ifds[0][259][0]) == 5 and int(ifds[0].get(317, [1])[0]) == predictor
        return os.pread(fd, int(ifds[0][279][0]), int(ifds[0][273][0]))
    finally:
        os.close(fd)


def build(name, spec, out, tmp):
    ifds, levels = [], tz.case_levels(name)
    for img in levels:
        h, w = img.shape[:2]
        tiles = tz.level_tiles(img, spec["tile"])
        streams = [tz.predict(t, 1) if spec["compression"] == 1 else libtiff_lzw(t, spec["predictor"], tmp) for t in tiles]
        ifds.append(tz.level_ifd(w, h, spec["tile"], streams, spec["compression"], spec["predictor"]))
    path = tz.fixture(name)
    wc.write_tiff(path, ifds, bigtiff=spec.get("bigtiff", False))
    with Image.open(path) as im:
        assert im.n_frames == len(levels)
        for i, img in enumerate(levels):
            im.seek(i)
            got = np.asarray(im.convert("RGB"))
            assert np.array_equal(got, img), (name, i)
            out[f"{name}/L{i}"] = got
    print(f"{name}: {os.path.getsize(path)} bytes")


def hostcheck(golden, tmp):
    run = tz.build_hostcheck(tmp, sanitize=False)
    work = os.path.join(tmp, "jobs")
    os.makedirs(work)
    jobs = {}
    for name in list(tz.CASES) + ["pipeline"]:
        with wsi.TiffSlide(tz.fixture(name)) as slide:
            for level in range(slide.level_count):
                jobs[(name, level)] = slide.tile_job(level)
                tz.write_job(os.path.join(work, f"{name}_L{level}.job"), jobs[(name, level)])
    print(run(work).strip())
    for (name, level), job in jobs.items():
        status, planes = tz.read_out(os.path.join(work, f"{name}_L{level}.out"), job)
        want = tz.tile_planes(tz.level_tiles(golden[f"{name}/L{level}"], tz.spec_of(name)["tile"]))[job["tiles"]]
        assert (status == 0).all() and np.array_equal(planes, want), (name, level, status)


def main():
    os.makedirs(tz.GOLDEN_DIR, exist_ok=True)
    out = {"pillow_version": np.array(PIL.__version__)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, spec in tz.CASES.items():
            build(name, spec, out, tmp)
        build("pipeline", tz.PIPELINE, out, tmp)
        np.savez_compressed(os.path.join(tz.GOLDEN_DIR, "tiffz.npz"), **out)
        print("tiffz.npz:", os.path.getsize(os.path.join(tz.GOLDEN_DIR, "tiffz.npz")), "bytes")
        hostcheck(out, tmp)


if __name__ == "__main__":
    main()
