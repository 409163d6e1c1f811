"""What the tests of the split (lane-parallel) JPEG entropy decode share: the sweep of subsequence sizes, the jobs of every
fixture, and the facts about the fixtures' scans that make the sweep reach the corners of the algorithm -- asserted from the
bytes of ``TiffSlide.tile_job`` on the host, so that a changed fixture cannot silently lose the coverage."""
import os

import numpy as np

import wsi_cases as wc
from sequoia_pub_amd import wsi

SWEEP = (0, 16, 20, 32, 64, 128)            # 0: the library's default
ALL = list(wc.CASES) + ["pipeline"]


def fixture(name):
    return os.path.join(wc.GOLDEN_DIR, f"{name}.tif")


def all_jobs():
    """{(case, level): tile_job} of every fixture and level."""
    jobs = {}
    for name in ALL:
        with wsi.TiffSlide(fixture(name)) as slide:
            for level in range(slide.level_count):
                jobs[(name, level)] = slide.tile_job(level)
    return jobs


def blocks_of(job):
    w, h, hs, vs = job["geom"]
    return (w // 8) * (h // 8) + 2 * (w // (8 * hs)) * (h // (8 * vs))


def boundary_counts(job, sub):
    """(subsequences that begin on the 00 of an FF 00 pair, subsequences that begin on an FF byte) over the job's scans."""
    on_zero = on_ff = 0
    scans = job["scans"]
    for off, length in job["table"][:, :2]:
        for q in range(int(off) + sub, int(off) + int(length), sub):
            on_zero += int(scans[q - 1] == 0xFF and scans[q] == 0)
            on_ff += int(scans[q] == 0xFF)
    return on_zero, on_ff


def assert_the_fixtures_reach_the_corners(jobs):
    noise, pipe = jobs[("noise100", 0)], jobs[("pipeline", 0)]
    assert (noise["table"][:, 3] == 0).all() and (pipe["table"][:, 3] == 0).all()              # no restart markers: these take the split path
    for sub in (16, 20, 32, 64):            # a boundary on the 00 of a stuffed pair, and one on an FF
        on_zero, on_ff = boundary_counts(noise, sub)
        assert on_zero > 0 and on_ff > 0, (sub, on_zero, on_ff)
        assert -(-int(noise["table"][:, 1].max()) // sub) > 64, sub                            # a second round of 64 with carried state
    assert boundary_counts(noise, 16) == (3, 8)
    # a block over at least four whole 16-byte subsequences (lanes that pass no block end): the longest block of the longest
    # scan has at least length / blocks bytes, and a run of n bytes holds (n - 15) // 16 whole subsequences wherever it starts
    assert blocks_of(noise) == 48 and (-(-int(noise["table"][:, 1].max()) // 48) - 15) // 16 >= 4
    # at least 15 block ends in one 16-byte subsequence: more blocks than 15 times the subsequences of a scan
    assert blocks_of(pipe) == 2048
    assert any(2048 > 14 * -(-int(n) // 16) for n in pipe["table"][:, 1])
    for sub in (16, 20):
        assert -(-int(pipe["table"][:, 1].max()) // sub) > 64, sub
    assert int(jobs[("single16", 0)]["table"][0, 1]) < 16                                      # a scan shorter than one subsequence
    assert len(jobs[("optimize", 0)]["sets"]) > 1                                              # tiles with tables of their own
    assert {j["geom"][2:] for j in jobs.values()} == {(1, 1), (2, 1), (2, 2)}                   # all three samplings
    assert (jobs[("ycc422", 0)]["table"][:, 3] > 0).all() and (jobs[("ycc444", 0)]["table"][:, 3] > 0).all()      # restart tiles


def repack(job, shift):
    """The job with every scan moved so that it starts at an offset congruent to `shift` modulo 16: (table, scans)."""
    table = job["table"].copy()
    parts, at = [], 0
    for slot, (off, length) in enumerate(job["table"][:, :2]):
        start = at + (shift - at) % 16
        parts.append(np.zeros(start - at, dtype=np.uint8))
        parts.append(job["scans"][int(off):int(off) + int(length)])
        table[slot, 0] = start
        at = start + int(length)
    parts.append(np.zeros(-at % 16, dtype=np.uint8))
    return table, np.concatenate(parts)
