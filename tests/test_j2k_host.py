"""CPU checks of the JPEG 2000 SVS reader: the codestream parser of sequoia_pub_amd.wsi on every fixture of tests/golden/j2k/
and its refusals, the upload ``tile_job`` prepares, and the decode core of csrc/j2k_core.h compiled for the host with the
address and undefined-behaviour sanitizers (tools/j2k_hostcheck.cpp, a stand-alone program) on every fixture -- against
Pillow's decode of the same streams under the parity rule of j2k_cases.check_parity -- and on damaged streams."""
import os
import struct

import numpy as np
import pytest

import j2k_cases as jc
import wsi_cases as wc
from sequoia_pub_amd import wsi
from sequoia_pub_amd._abi import CONSTANTS as C

ALL = list(jc.CASES) + ["pipeline"]
ORDERS = {"LRCP": 0, "RLCP": 1, "RPCL": 2, "PCRL": 3, "CPRL": 4}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(jc.GOLDEN_DIR, "j2k.npz"))


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return jc.build_hostcheck(tmp_path_factory.mktemp("j2k_hostcheck"), sanitize=True)


def first_stream(name):
    with wsi.TiffSlide(jc.fixture(name)) as slide:
        offsets, counts = slide.tile_ranges(0)
    raw = open(jc.fixture(name), "rb").read()
    return raw[int(offsets[0]):int(offsets[0]) + int(counts[0])]


@pytest.mark.parametrize("name", ALL)
def test_parser_accepts_every_case_and_tile_job_needs_no_gpu(name):
    spec = jc.spec_of(name)
    opts = spec["opts"]
    with wsi.TiffSlide(jc.fixture(name)) as slide:
        assert slide.level_dimensions == tuple(spec["levels"]) and slide.bigtiff == spec.get("bigtiff", False)
        assert slide.properties["openslide.vendor"] == "aperio" and slide.properties["aperio.AppMag"] == "20"
        assert "J2K/KDU" in slide.properties["tiff.ImageDescription"]
        h = wsi.parse_j2k(first_stream(name), name)
        assert h.size == spec["tile"] and h.dx == (2 if spec.get("s422") else 1)
        assert h.levels == opts["num_resolutions"] - 1 and h.reversible == (not opts["irreversible"])
        assert h.mct == (0 if spec.get("s422") else opts.get("mct", 0)) and h.layers == len(opts.get("quality_layers", [0]))
        assert h.order == (4 if spec.get("s422") else ORDERS[opts.get("progression", "LRCP")])
        assert (1 << h.xcb, 1 << h.ycb) == tuple(opts.get("codeblock_size", (64, 64)))
        if "precinct_size" in opts:
            assert h.precincts[-1] == (6, 6)
        else:
            assert h.precincts == [(15, 15)] * (h.levels + 1)
        styles = [q[1] for q in h.quant]
        want = 0 if h.reversible else 2
        assert styles == {"qcd": [1, 1, 1], "qcc": [2, 1, 2]}.get(spec.get("derived"), [want] * 3)
        assert len(h.params) == C["SQ_J2K_PARAM_BYTES"]
        for level, (w, hgt) in enumerate(spec["levels"]):
            n = -(-w // spec["tile"][0]) * -(-hgt // spec["tile"][1])
            job = slide.tile_job(level)
            assert job["codec"] == "j2k" and job["geom"] == spec["tile"] + (1, 1)
            assert job["transform"] == (spec["compression"] == 33003) and sorted(job["tiles"]) == list(range(n))
            assert job["table"].shape == (n, C["SQ_J2K_TILE_WORDS"]) and (np.diff(job["table"][:, 1]) <= 0).all()
            assert len(job["sets"]) == 1 and len(job["scans"]) % 16 == 0 and min(job["caps"]) >= 1       # equal headers share one set
            offsets, counts = slide.tile_ranges(level)
            raw = open(jc.fixture(name), "rb").read()
            for slot, t in enumerate(job["tiles"]):        # the packet bytes: what lies between SOD and EOC in the file
                a, length = int(job["table"][slot, 0]), int(job["table"][slot, 1])
                stream = raw[int(offsets[t]):int(offsets[t]) + int(counts[t])]
                sod = stream.index(b"\xff\x93")
                assert job["scans"][a:a + length].tobytes() == stream[sod + 2:len(stream) - 2] and stream[-2:] == b"\xff\xd9"


def test_jpeg_levels_still_say_their_codec():
    with wsi.TiffSlide(os.path.join(wc.GOLDEN_DIR, "ycc420.tif")) as slide:
        assert slide.tile_job(0)["codec"] == "jpeg"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def patched(data, marker, offset, value):
    """`data` with the byte at `offset` of the payload (behind the length) of segment `marker` replaced."""
    a, _ = jc.segment(data, marker)
    out = bytearray(data)
    out[a + 4 + offset] = value
    return bytes(out)


def inserted(data, marker, payload, before=0x52):
    a, _ = jc.segment(data, before)
    return data[:a] + bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload + data[a:]


def refusals():
    base = first_stream("cb32")                  # 64 x 64, 3 levels, LRCP, maximal precincts
    prec = first_stream("precinct")
    out = {}
    for bit, text in enumerate(["bypass", "reset", "termination on each", "vertically causal", "predictable termination", "segmentation symbols"]):
        out[f"style_{bit}"] = (patched(base, 0x52, 8, 1 << bit), rf"COD code-block style {1 << bit:#x} \(.*{text}")
    out["sop"] = (patched(base, 0x52, 0, 2), r"COD Scod = 0x2: SOP")
    out["eph"] = (patched(base, 0x52, 0, 4), r"COD Scod = 0x4: EPH")
    out["poc"] = (inserted(base, 0x5F, bytes(7)), r"POC marker segment \(0x5f\)")
    out["rgn"] = (inserted(base, 0x5E, bytes(3)), r"RGN marker segment \(0x5e\)")
    out["ppm"] = (inserted(base, 0x60, bytes(3)), r"PPM marker segment \(0x60\)")
    out["ppt"] = (inserted(base, 0x61, bytes(3), before=0x93), r"PPT marker segment \(0x61\)")
    out["tlm"] = (inserted(base, 0x55, bytes(4)), r"TLM marker segment \(0x55\)")
    a, _ = jc.segment(base, 0x51)
    two_tiles = bytearray(base)
    struct.pack_into(">I", two_tiles, a + 4 + 18, 32)                      # XTsiz = 32 in an image of 64
    out["tiles"] = (bytes(two_tiles), r"SIZ tiles of 32 x 64 in an image of 64 x 64: more than one tile")
    out["tile_part"] = (patched(base, 0x90, 7, 2), r"SOT tile 0, tile-part 0 of 2")
    out["depth"] = (patched(base, 0x51, 36, 11), r"SIZ Ssiz = \[11, 7, 7\]")
    out["signed"] = (patched(base, 0x51, 36, 0x87), r"SIZ Ssiz = \[135, 7, 7\]")
    out["components"] = (patched(base, 0x51, 35, 4), r"SIZ Csiz = 4 components")
    out["sampling"] = (patched(base, 0x51, 38, 2), r"SIZ component sampling \(XRsiz, YRsiz\) = \[\(1, 2\)")
    out["offset"] = (patched(base, 0x51, 13, 1), r"SIZ image and tile offsets \(1, 0, 0, 0\)")
    out["block_128"] = (patched(base, 0x52, 6, 5), r"COD code-block size 128 x 32")
    out["levels"] = (patched(base, 0x52, 5, 9), r"COD with 9 decomposition levels")
    out["wavelet"] = (patched(base, 0x52, 9, 2), r"COD wavelet 2")
    out["order"] = (patched(base, 0x52, 1, 5), r"COD progression order 5")
    out["layers"] = (patched(base, 0x52, 3, 33), r"COD with 33 quality layers")
    out["positional"] = (patched(prec, 0x52, 1, 2), r"COD progression RPCL with 4 precincts at resolution 0")
    out["quant_style"] = (patched(base, 0x5C, 0, 0x43), r"QCD quantisation style 3")
    out["coc"] = (inserted(base, 0x53, bytes([1, 0, 2, 4, 4, 0, 0]), before=0x5C), r"COC for component 1 differs from COD")
    out["mct_422"] = (patched(first_stream("odd422"), 0x52, 4, 1), r"multiple component transform with SIZ sampling 2x1")
    out["no_siz"] = (base[:2] + base[jc.segment(base, 0x51)[1]:], r"SOD without SIZ")
    out["jp2"] = (b"\x00\x00\x00\x0cjP  \r\n\x87\n" + base, r"no SOC marker")
    return out


REFUSALS = refusals()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_parser_refuses_naming_the_marker_or_field(name):
    data, match = REFUSALS[name]
    with pytest.raises(wsi.WsiFormatError, match=match):
        wsi.parse_j2k(data, name)


def test_container_refusals(tmp_path):
    path = str(tmp_path / "bad.tif")
    good = first_stream("single16")

    def refuse(match, ifd):
        wc.write_tiff(path, [ifd])
        with pytest.raises(wsi.WsiFormatError, match=match):
            wsi.TiffSlide(path)
    refuse(r"Compression = 34712 \(JPEG 2000\) is not supported", wc.level_ifd(16, 16, 16, [good], 2, 0, compression=34712))
    refuse(r"Compression = 8 \(deflate\) is not supported", wc.level_ifd(16, 16, 16, [good], 2, 0, compression=8))
    # a JPEG stream under the JPEG 2000 compression, and a JP2 file: what was found instead of a codestream is named
    jpeg = open(os.path.join(wc.GOLDEN_DIR, "single16.tif"), "rb").read()
    soi = jpeg.index(b"\xff\xd8")
    refuse(r"IFD 0: Compression = 33005 \(Aperio JPEG 2000, RGB\) but .* holds a JPEG stream \(SOI\)",
           wc.level_ifd(16, 16, 16, [jpeg[soi:soi + 200]], 2, 0, compression=33005))
    refuse(r"IFD 0: Compression = 33003 \(Aperio JPEG 2000, YCbCr\) but .* holds a JP2 file",
           wc.level_ifd(16, 16, 16, [b"\x00\x00\x00\x0cjP  \r\n\x87\n" + good], 6, 0, compression=33003))
    refuse(r"SIZ image of 16 x 16 pixels in tiles of 32 x 32", wc.level_ifd(32, 32, 32, [good], 2, 0, compression=33005))
    # the photometric tag is not consulted: 33005 with photometric 6 opens, components as stored
    wc.write_tiff(path, [wc.level_ifd(16, 16, 16, [good], 6, 0, compression=33005)])
    with wsi.TiffSlide(path) as slide:
        assert slide.tile_job(0)["transform"] == 0


# ---- the host build of the core ---------------------------------------------------------------------------------------------
def test_host_build_of_the_core_meets_the_parity_rule_under_sanitizers(hostcheck, golden, tmp_path):
    jobs = {}
    for name in ALL:
        with wsi.TiffSlide(jc.fixture(name)) as slide:
            for level in range(slide.level_count):
                jobs[(name, level)] = slide.tile_job(level)
                jc.write_job(tmp_path / f"{name}_L{level}.job", jobs[(name, level)])
    assert f"{len(jobs)} job(s), 0 failed" in hostcheck(tmp_path)
    for (name, level), job in jobs.items():
        status, planes = jc.read_out(tmp_path / f"{name}_L{level}.out", job)
        assert (status == 0).all(), (name, level, status)
        jc.check_parity(planes, golden[f"{name}/L{level}/tiles"][job["tiles"]], jc.spec_of(name).get("exact", False), f"{name} L{level}")


def test_damaged_streams_give_their_status_and_a_clean_sanitizer_run(hostcheck, tmp_path):
    """Every case holds the four tiles of 'rct' (lossless: every packet has a body); slot 0 is damaged, the others must decode
    as in the good job."""
    with wsi.TiffSlide(jc.fixture("rct")) as slide:
        job = slide.tile_job(0)
    a, length = int(job["table"][0, 0]), int(job["table"][0, 1])
    cases = {}
    cut = job["table"].copy()
    cut[0, 1] = 1                                   # the first packet header needs more than a byte
    cases["cut_in_header"] = (cut, None, C["SQ_J2K_TRUNCATED_HEADER"])
    cut = job["table"].copy()
    cut[0, 1] = length - 1                          # the last packet's body lacks a byte
    cases["cut_in_body"] = (cut, None, C["SQ_J2K_TRUNCATED_BODY"])
    scans = job["scans"].copy()
    scans[a:a + len(jc.LENGTH_PAST_STREAM)] = np.frombuffer(jc.LENGTH_PAST_STREAM, dtype=np.uint8)
    cases["length_past_stream"] = (None, scans, C["SQ_J2K_BAD_LENGTH"])
    scans = job["scans"].copy()
    scans[a:a + length] = 0                         # every packet reads as empty: no block has a byte, the planes are flat
    cases["emptied"] = (None, scans, C["SQ_J2K_OK"])
    scans = job["scans"].copy()
    assert scans[a] & 0x80
    scans[a] ^= 0x80                                # the first packet reads as empty and its bytes as the next headers
    cases["flipped_bit"] = (None, scans, None)
    past = job["table"].copy()
    past[0, 0] = len(job["scans"]) - 2
    cases["range_past_end"] = (past, None, C["SQ_J2K_BAD_RANGE"])
    bad_set = job["table"].copy()
    bad_set[0, 2] = 3
    cases["no_such_set"] = (bad_set, None, C["SQ_J2K_BAD_PARAM"])
    jc.write_job(tmp_path / "good.job", job)
    for name, (table, scans, _) in cases.items():
        jc.write_job(tmp_path / f"{name}.job", job, table=table, scans=scans)
    small = dict(job, caps=(job["caps"][0] - 1,) + tuple(job["caps"][1:]))          # records for one block less than the set needs
    jc.write_job(tmp_path / "small_caps.job", small)
    hostcheck(tmp_path)
    ok_status, ok_planes = jc.read_out(tmp_path / "good.out", job)
    assert (ok_status == 0).all()
    for name, (_, _, expect) in cases.items():
        status, planes = jc.read_out(tmp_path / f"{name}.out", job)
        if expect is None:
            assert 0 <= status[0] <= C["SQ_J2K_TRUNCATED_BODY"], (name, status)
        else:
            assert status[0] == expect, (name, status)
        if status[0] != 0:
            assert (planes[0] == 0).all(), name                                     # the planes of a failing tile are zero
        assert (status[1:] == 0).all() and np.array_equal(planes[1:], ok_planes[1:]), (name, status)
    assert (jc.read_out(tmp_path / "emptied.out", job)[1][0] == 128).all()
    status, _ = jc.read_out(tmp_path / "small_caps.out", job)
    assert (status == C["SQ_J2K_BAD_PARAM"]).all()


def test_the_damaged_file_of_the_gpu_test_runs_clean_on_the_host(hostcheck, tmp_path):
    expect = jc.damage_file(jc.fixture("rct"), str(tmp_path / "damaged.tif"))
    with wsi.TiffSlide(str(tmp_path / "damaged.tif")) as slide:
        job = slide.tile_job(0)
    jc.write_job(tmp_path / "damaged.job", job)
    hostcheck(tmp_path)
    status, _ = jc.read_out(tmp_path / "damaged.out", job)
    assert {t: int(status[s]) for s, t in enumerate(job["tiles"])} == {0: 0, 3: 0, **{t: C[v] for t, v in expect.items()}}
