"""Regenerates tests/golden/wsi_jobs.json: what ``TiffSlide.read_regions`` uploads for every level of every slide fixture under
tests/golden/wsi/, tests/golden/j2k/ and tests/golden/tiffz/, as recorded results (wsi_cases.job_records).

    "<directory>/<name>": [per level
        {"tile_ranges": SHA-256 of the level's TileOffsets and TileByteCounts (int64, little-endian),
         "all":  tile_job(level),
         "half": tile_job(level, tiles=<every second tile, in descending order>)}]
    a job: codec, geom, tiles (the tile number of every slot), transform / predictor / caps where the codec has them, the shape
    of the table, and the SHA-256 of table.tobytes(), of b"".join(sets) and of scans.tobytes()

The file pins the slot order (ties included), the table rows, the padding and the de-duplication of the table sets: it is made
once, by the reader as it stands, BEFORE a change that must leave the upload alone, and tests/test_wsi_host.py compares the
reader against it from then on.  Made anew only when the upload is meant to change.  Needs the built library (sq_j2k_layout
sizes the JPEG 2000 caps), no GPU.

    python tests/golden/make_wsi_jobs_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import wsi_cases as wc  # noqa: E402
from sequoia_pub_amd import wsi  # noqa: E402


def main():
    out = {}
    for name in wc.job_fixtures():
        with wsi.TiffSlide(os.path.join(HERE, name + ".tif")) as slide:
            out[name] = wc.job_records(slide)
    with open(wc.JOBS_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{wc.JOBS_GOLDEN}: {len(out)} slides, {sum(map(len, out.values()))} levels, {os.path.getsize(wc.JOBS_GOLDEN)} bytes")


if __name__ == "__main__":
    main()
