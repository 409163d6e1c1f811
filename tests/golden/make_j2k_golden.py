"""Regenerates tests/golden/j2k/ and profiles/j2k_parity.txt: the JPEG 2000 SVS fixtures of tests/j2k_cases.py and j2k.npz
with Pillow's (OpenJPEG's) decode of every tile stream:

    <case>.tif               the fixture (tiles encoded by Pillow, 4:2:2 and derived quantisation by the constructions of
                             j2k_cases, the container written by wsi_cases.write_tiff)
    <case>/L<i>/tiles        uint8 [n, 3, tile_h, tile_w]   the component planes of every tile as Pillow decodes its stream
                                                            (4:2:2: the three stand-alone decodes, chroma repeated)
    pipeline.tif, pipeline/L<i>/tiles   the synthetic slide of the pipeline tests (lossless)

Then it builds tools/j2k_hostcheck.cpp with the host compiler, runs every case through it, checks the parity rule, asserts
that the noise case reaches all 19 MQ contexts (the run-length and uniform contexts among them) and writes the measured
share of differing bytes and the largest difference per case to profiles/j2k_parity.txt.

    python tests/golden/make_j2k_golden.py
"""
import io
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import j2k_cases as jc  # noqa: E402
import wsi_cases as wc  # noqa: E402


def build(name, spec, out):
    levels = jc.case_levels(name)
    tw, th = spec["tile"]
    ifds = []
    for i, img in enumerate(levels):
        h, w = img.shape[:2]
        streams, planes = [], []
        for ty in range(-(-h // th)):
            for tx in range(-(-w // tw)):
                s, p = jc.encode_tile(jc.pad_tile(img, tx, ty, spec["tile"]), spec)
                streams.append(s)
                planes.append(p)
                if spec.get("s422"):                # Pillow opens the joined stream as one full-size image of three components
                    with Image.open(io.BytesIO(s)) as joined:
                        assert joined.size == (tw, th) and len(joined.getbands()) == 3, (name, joined.size, joined.getbands())
        out[f"{name}/L{i}/tiles"] = np.stack(planes)
        desc = jc.APERIO.format(w=w, h=h, tw=tw, th=th) if i == 0 else None
        tags = wc.level_ifd(w, h, tw, streams, 6 if spec["compression"] == 33003 else 2, 1 if spec.get("s422") else 0, None, desc,
                            compression=spec["compression"])
        tags[323] = (4, th)
        ifds.append(tags)
    path = jc.fixture(name)
    wc.write_tiff(path, ifds, bigtiff=spec.get("bigtiff", False))
    print(f"{name}: {os.path.getsize(path)} bytes")


def parity(golden):
    """Every case through the host build of csrc/j2k_core.h; returns the lines of profiles/j2k_parity.txt."""
    from sequoia_pub_amd import wsi
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "j2k_hostcheck")
        subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "j2k_hostcheck.cpp")], check=True)
        for name in list(jc.CASES) + ["pipeline"]:
            spec = jc.spec_of(name)
            work = os.path.join(tmp, name)
            os.makedirs(work)
            with wsi.TiffSlide(jc.fixture(name)) as slide:
                jobs = [slide.tile_job(level) for level in range(slide.level_count)]
            for level, job in enumerate(jobs):
                jc.write_job(os.path.join(work, f"L{level}.job"), job)
            r = subprocess.run([exe, work, "--hits"], capture_output=True, text=True, check=True)
            hits = [int(v) for v in r.stdout.split("contexts:")[1].split()]
            share, worst, total = 0.0, 0, 0
            for level, job in enumerate(jobs):
                status, planes = jc.read_out(os.path.join(work, f"L{level}.out"), job)
                assert (status == 0).all(), (name, level, status)
                want = golden[f"{name}/L{level}/tiles"][job["tiles"]]
                s, m = jc.check_parity(planes, want, spec.get("exact", False), f"{name} L{level}")
                share, worst, total = share + s * planes.size, max(worst, m), total + planes.size
            if name == "noise":                     # the case exists for this: it must keep reaching every context
                assert len(hits) == 19 and min(hits) > 0, hits
                lines.append(f"# noise: uses of MQ contexts 0..18: {' '.join(map(str, hits))}")
            rule = "equal" if spec.get("exact") else "within 1, share <= 0.01"
            lines.append(f"{name:10s} bytes {total:8d}  differing share {share / total:.6f}  largest difference {worst}  ({rule})")
    return lines


def main():
    os.makedirs(jc.GOLDEN_DIR, exist_ok=True)
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, spec in jc.CASES.items():
        build(name, spec, out)
    build("pipeline", jc.PIPELINE, out)
    np.savez_compressed(os.path.join(jc.GOLDEN_DIR, "j2k.npz"), **out)
    print("j2k.npz:", os.path.getsize(os.path.join(jc.GOLDEN_DIR, "j2k.npz")), "bytes")
    lines = parity(out)
    with open(os.path.join(ROOT, "profiles", "j2k_parity.txt"), "w") as f:
        f.write("# Host build of csrc/j2k_core.h (tools/j2k_hostcheck.cpp, -ffp-contract=off) against Pillow "
                f"{PIL.__version__}'s OpenJPEG decode of the same tile streams,\n# component planes of every tile of every level "
                "(tests/golden/make_j2k_golden.py).  CPU only: no GPU run is behind these figures.\n")
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
