"""CPU checks of the split (lane-parallel) JPEG entropy decode: the lane-level functions of csrc/jpeg_core.h driven by
tools/jpegsplit_hostcheck.cpp as the device kernel drives them (the 64 lanes a loop), built stand-alone with the address and
undefined-behaviour sanitizers, against the Pillow-made goldens and against the serial program's output byte for byte, on every
fixture over the sweep of subsequence sizes and on the damaged streams of tests/test_wsi_host.py; and the argument checks of
the Python layer that need no GPU."""
import os
import re
import shutil

import numpy as np
import pytest

import wsi_cases as wc
import wsi_split_cases as sc
from test_wsi_host import damaged_jobs, read_out, write_job
from sequoia_pub_amd import wsi
from sequoia_pub_amd._abi import CONSTANTS as C


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(wc.GOLDEN_DIR, "wsi.npz"))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """Both stand-alone programs built with the host compiler and the sanitizers: run(which, directory, *args) -> stdout."""
    build = tmp_path_factory.mktemp("splitcheck")
    runners = {name: wc.build_hostcheck(f"{name}.cpp", build, sanitize=True) for name in ("jpegsplit_hostcheck", "jpegdec_hostcheck")}
    return lambda which, directory, *args: runners[which](directory, *args)


@pytest.fixture(scope="module")
def sweep(programs, tmp_path_factory):
    """Every fixture and level through the serial program once and through the split program at every size of the sweep:
    (jobs, directory of the serial run, {sub_bytes: (directory, {job name: (sync rounds, fallbacks)})})."""
    jobs = sc.all_jobs()
    sc.assert_the_fixtures_reach_the_corners(jobs)
    serial = tmp_path_factory.mktemp("serial")
    for (name, level), job in jobs.items():
        write_job(serial / f"{name}_L{level}.job", job)
    assert f"{len(jobs)} job(s), 0 failed" in programs("jpegdec_hostcheck", serial)
    runs = {}
    for sub in sc.SWEEP:
        d = tmp_path_factory.mktemp(f"split{sub}")
        for f in os.listdir(serial):
            if f.endswith(".job"):
                shutil.copy(serial / f, d / f)
        out = programs("jpegsplit_hostcheck", d, sub)
        assert f"{len(jobs)} job(s), 0 failed" in out
        runs[sub] = (d, {m[0]: (int(m[1]), int(m[2])) for m in re.findall(r"^(\w+): sync_rounds (\d+) fallbacks (\d+)$", out, flags=re.M)})
        assert len(runs[sub][1]) == len(jobs)
    return jobs, serial, runs


def test_host_build_of_the_split_decode_equals_the_goldens_and_the_serial_program(sweep, golden):
    jobs, serial, runs = sweep
    for sub, (d, _) in runs.items():
        for (name, level), job in jobs.items():
            status, rgb = read_out(d / f"{name}_L{level}.out", job)
            assert (status == 0).all(), (sub, name, level, status)
            if name != "pipeline":          # its golden holds levels, not tiles: the serial program's bytes stand for it
                want = golden[f"{name}/L{level}/tiles"].transpose(0, 2, 3, 1)[job["tiles"]]
                assert np.array_equal(rgb, want), (sub, name, level)
            assert open(d / f"{name}_L{level}.out", "rb").read() == open(serial / f"{name}_L{level}.out", "rb").read(), (sub, name, level)


def test_the_default_is_a_size_the_entry_takes():
    d = C["SQ_JPEG_SPLIT_SUB_DEFAULT"]
    assert C["SQ_JPEG_SPLIT_SUB_MIN"] == 16 and C["SQ_JPEG_SPLIT_SUB_MAX"] >= 256
    assert C["SQ_JPEG_SPLIT_SUB_MIN"] <= d <= C["SQ_JPEG_SPLIT_SUB_MAX"] and d % 4 == 0


def test_synchronisation_is_exercised_and_no_clean_job_falls_back(sweep):
    jobs, _, runs = sweep
    most = {(name, sub): rounds for sub, (_, report) in runs.items() for name, (rounds, _) in report.items()}
    print("synchronisation rounds:", {k: v for k, v in most.items() if v >= 2})
    assert max(most.values()) >= 2, most
    for sub, (_, report) in runs.items():
        for (name, level), job in jobs.items():
            with_restart = int((job["table"][:, 3] > 0).sum())
            assert report[f"{name}_L{level}"][1] == with_restart, (sub, name, level, report[f"{name}_L{level}"])


@pytest.mark.parametrize("sub", [16, 64])
def test_damaged_streams_equal_the_serial_program_under_the_sanitizers(programs, tmp_path, sub):
    cases = damaged_jobs()
    good = {}
    for name, (job, table, sets, scans, expect) in cases.items():
        write_job(tmp_path / f"{name}.job", job, table, sets, scans)
        if id(job) not in good:
            good[id(job)] = f"good{len(good)}"
            write_job(tmp_path / f"{good[id(job)]}.job", job)
    programs("jpegdec_hostcheck", tmp_path)
    serial = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path) if f.endswith(".out")}
    for f in serial:
        os.remove(tmp_path / f)
    programs("jpegsplit_hostcheck", tmp_path, sub)
    assert len(serial) == len(cases) + len(good)
    for f, want in serial.items():
        assert open(tmp_path / f, "rb").read() == want, (sub, f)               # statuses and every pixel
    for name, (job, table, sets, scans, expect) in cases.items():
        status, rgb = read_out(tmp_path / f"{name}.out", job)
        ok_status, ok_rgb = read_out(tmp_path / f"{good[id(job)]}.out", job)
        assert (ok_status == 0).all()
        for slot in range(len(status)):
            if slot in expect:
                assert status[slot] == expect[slot], (name, slot, status)
            else:                           # untouched tiles are unaffected
                assert status[slot] == 0 and np.array_equal(rgb[slot], ok_rgb[slot]), (name, slot, status)


def test_scans_at_any_byte_on_the_host(programs, tmp_path):
    """noise100 re-packed so that its scans start at 1, 2, 3 and 15 modulo 16: the chunk walks of the lanes, under the sanitizers."""
    with wsi.TiffSlide(sc.fixture("noise100")) as slide:
        job = slide.tile_job(0)
    write_job(tmp_path / "shift0.job", job)
    for shift in (1, 2, 3, 15):
        table, scans = sc.repack(job, shift)
        assert (table[:, 0] % 16 == shift).all() and len(scans) % 16 == 0
        write_job(tmp_path / f"shift{shift}.job", job, table=table, scans=scans)
    programs("jpegsplit_hostcheck", tmp_path, 16)
    want = open(tmp_path / "shift0.out", "rb").read()
    for shift in (1, 2, 3, 15):
        assert open(tmp_path / f"shift{shift}.out", "rb").read() == want, shift


def test_entropy_argument_is_checked_at_construction():
    for bad in ("both", "", None, "Split"):
        with pytest.raises(ValueError, match="entropy"):
            wsi.TiffSlide(sc.fixture("single16"), entropy=bad)
    with pytest.raises(ValueError, match="sub_bytes"):
        wsi.TiffSlide(sc.fixture("single16"), entropy="split", sub_bytes=18)
    with pytest.raises(ValueError, match="entropy"):
        wsi.open_slide(sc.fixture("single16"), reader="tiff", entropy="both")
    with wsi.TiffSlide(sc.fixture("single16")) as slide:
        assert slide.entropy == "serial" and slide.sub_bytes == 0
    with wsi.TiffSlide(sc.fixture("single16"), entropy="split", sub_bytes=32) as slide:
        assert slide.entropy == "split" and slide.sub_bytes == 32
    with wsi.open_slide(sc.fixture("single16"), reader="tiff", entropy="split") as slide:
        assert slide.entropy == "split"


def test_the_clis_take_the_flag_and_default_to_serial():
    from sequoia_pub_amd.cli import patch_gen_hdf5, slide_features, visualize
    for mod in (patch_gen_hdf5, slide_features, visualize):
        parser = mod.build_parser()
        required = [a for action in parser._actions if action.required for a in (action.option_strings[0], "x")]
        assert parser.parse_args(required).jpeg_entropy == "serial", mod.__name__
        assert parser.parse_args(required + ["--jpeg_entropy", "split"]).jpeg_entropy == "split", mod.__name__
        with pytest.raises(SystemExit):
            parser.parse_args(required + ["--jpeg_entropy", "both"])
