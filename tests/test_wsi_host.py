"""CPU checks of the JPEG-tiled TIFF / SVS reader: the numpy restatement of the decode against the Pillow-made goldens (and
live Pillow where it has JPEG and libtiff), the container parser against the fixtures' known structure (and Pillow's tag_v2),
the decode core of csrc/jpeg_core.h compiled for the host with the address and undefined-behaviour sanitizers
(tools/jpegdec_hostcheck.cpp, a stand-alone program) on every fixture and on damaged streams, and the parser's refusals."""
import io
import os
import struct

import numpy as np
import pytest

import wsi_cases as wc
from sequoia_pub_amd import wsi
from sequoia_pub_amd._abi import CONSTANTS as C

ALL = list(wc.CASES) + ["pipeline"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(wc.GOLDEN_DIR, "wsi.npz"))


def spec_of(name):
    return wc.PIPELINE if name == "pipeline" else wc.CASES[name]


def fixture(name):
    return os.path.join(wc.GOLDEN_DIR, f"{name}.tif")


def tile_streams(path, slide, level):
    """The full stand-alone stream of every tile of a level: JPEGTables joined in front of the tile's bytes."""
    offsets, counts = slide.tile_ranges(level)
    raw = open(path, "rb").read()
    ifds, _ = wsi.read_ifds(slide._fd, slide._size)
    tables = ifds[slide._levels[level].index].get(347)
    return [wc.join_tables(None if tables is None else bytes(tables), raw[o:o + c]) for o, c in zip(offsets, counts)]


def assemble(tiles_rgb, width, height, tile):
    """Tiles [n, tile, tile, 3] row-major -> the level image, cropped as libtiff crops it."""
    tx = -(-width // tile)
    out = np.zeros((height, width, 3), dtype=np.uint8)
    for t, img in enumerate(tiles_rgb):
        y, x = (t // tx) * tile, (t % tx) * tile
        out[y:y + tile, x:x + tile] = img[:height - y, :width - x]
    return out


@pytest.mark.parametrize("name", list(wc.CASES))
def test_numpy_restatement_equals_pillow_goldens(name, golden):
    spec = wc.CASES[name]
    with wsi.TiffSlide(fixture(name)) as slide:
        assert slide.level_dimensions == tuple(spec["levels"])
        for level, (w, h) in enumerate(spec["levels"]):
            streams = tile_streams(fixture(name), slide, level)
            mine = np.stack([wc.decode_tile(s, spec["photometric"] == 6) for s in streams])
            assert np.array_equal(mine, golden[f"{name}/L{level}/tiles"].transpose(0, 2, 3, 1))          # libjpeg-turbo, per tile
            assert np.array_equal(assemble(mine, w, h, spec["tile"]), golden[f"{name}/L{level}"].transpose(1, 2, 0))      # libtiff, the level


def test_noise_case_still_covers_stuffing_zero_runs_and_long_codes():
    with wsi.TiffSlide(fixture("noise100")) as slide:
        events = dict(stuffed=0, zrl=0, long_codes=0)
        for s in tile_streams(fixture("noise100"), slide, 0):
            ev = {}
            wc.decode_tile(s, True, ev)
            for k in events:
                events[k] += ev[k]
    assert events["stuffed"] > 0 and events["zrl"] > 0 and events["long_codes"] > 0, events


def test_goldens_equal_live_pillow_where_it_has_jpeg_and_libtiff(golden):
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not (features.check("jpg") and features.check("libtiff")):
        pytest.skip("Pillow without JPEG or libtiff")
    for name in wc.CASES:
        with wsi.TiffSlide(fixture(name)) as slide:
            for t, s in enumerate(tile_streams(fixture(name), slide, 0)):
                live = np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))
                assert np.array_equal(live, golden[f"{name}/L0/tiles"][t].transpose(1, 2, 0)), (name, t)


@pytest.mark.parametrize("name", ALL)
def test_container_parser(name):
    spec = spec_of(name)
    with wsi.TiffSlide(fixture(name)) as slide:
        assert slide.bigtiff == spec["bigtiff"]
        assert slide.level_count == len(spec["levels"]) and slide.dimensions == tuple(spec["levels"][0])
        assert slide.level_dimensions == tuple(spec["levels"])                       # stripped IFDs are no levels
        assert slide.level_downsamples == tuple(spec["levels"][0][0] / w for w, _ in spec["levels"])
        assert slide.properties["openslide.vendor"] == "aperio" and slide.properties["aperio.AppMag"] == "20"
        assert slide.properties["aperio.MPP"] == slide.properties["openslide.mpp-x"] == slide.properties["openslide.mpp-y"] == "0.5021"
        assert slide.properties["aperio.Filename"] == "synthetic"
        assert slide.properties["openslide.level-count"] == str(len(spec["levels"]))             # a string, as OpenSlide's
        size = os.path.getsize(fixture(name))
        for level, (w, h) in enumerate(spec["levels"]):
            offsets, counts = slide.tile_ranges(level)
            n = -(-w // spec["tile"]) * -(-h // spec["tile"])
            assert len(offsets) == len(counts) == n and (counts > 0).all() and (offsets + counts <= size).all()
            job = slide.tile_job(level)
            assert job["geom"] == (spec["tile"], spec["tile"]) + wc.SAMPLING[spec["subsampling"]]
            assert job["transform"] == (spec["photometric"] == 6) and sorted(job["tiles"]) == list(range(n))
            assert (np.diff(job["table"][:, 1]) <= 0).all()                          # longest scan first
            assert (job["table"][:, 3] == spec["restart"]).all()
            if spec["optimize"]:                    # every tile carries Huffman tables made for it: more than one distinct set
                assert 1 < len(job["sets"]) <= n and len(set(job["sets"])) == len(job["sets"])
            else:                                   # one JPEGTables stream: one set, and one object behind every tile
                assert len(job["sets"]) == 1
                assert len({id(slide._tile_info(slide._levels[level], t)[2]) for t in range(n)}) == 1


def test_container_parser_agrees_with_pillow_tag_v2():
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("Pillow without libtiff")
    for name in ALL:
        with wsi.TiffSlide(fixture(name)) as slide, Image.open(fixture(name)) as im:
            ifds, _ = wsi.read_ifds(slide._fd, slide._size)
            assert im.n_frames == len(ifds)
            for frame, tags in enumerate(ifds):
                im.seek(frame)
                for tag in (256, 257, 259, 262, 277, 322, 323):
                    if tag in tags or tag in im.tag_v2:
                        assert int(tags[tag][0]) == int(np.ravel(im.tag_v2[tag])[0]), (name, frame, tag)
                for tag in (324, 325):
                    if tag in tags:
                        assert [int(v) for v in tags[tag]] == [int(v) for v in im.tag_v2[tag]], (name, frame, tag)
                if 270 in tags:
                    assert tags[270].split(b"\0")[0].decode("latin-1") == im.tag_v2[270]


def test_generic_tiff_without_description_gives_the_default_magnification(tmp_path):
    spec = wc.CASES["single16"]
    with wsi.TiffSlide(fixture("single16")) as slide:
        offsets, counts = slide.tile_ranges(0)
        ifds, _ = wsi.read_ifds(slide._fd, slide._size)
    raw = open(fixture("single16"), "rb").read()
    tile = raw[offsets[0]:offsets[0] + counts[0]]
    path = str(tmp_path / "plain.tif")
    wc.write_tiff(path, [wc.level_ifd(16, 16, 16, [tile], 6, spec["subsampling"], bytes(ifds[0][347]))])
    with wsi.TiffSlide(path) as slide:
        assert slide.properties["openslide.vendor"] == "generic-tiff" and "aperio.AppMag" not in slide.properties
        assert float(slide.properties.get("aperio.AppMag", 20)) == 20.0


def test_the_upload_of_every_fixture_level_equals_the_recorded_jobs():
    """Slot order (ties included), table rows, padding, set de-duplication and scans of every level of every slide fixture --
    JPEG, JPEG 2000, LZW and uncompressed -- against tests/golden/wsi_jobs.json (tests/golden/make_wsi_jobs_golden.py)."""
    import json
    with open(wc.JOBS_GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(wc.job_fixtures())
    for name in wc.job_fixtures():
        with wsi.TiffSlide(os.path.join(os.path.dirname(wc.GOLDEN_DIR), name + ".tif")) as slide:
            got = wc.job_records(slide)
        assert len(got) == len(want[name]), name
        for level, (g, w) in enumerate(zip(got, want[name])):
            assert g == w, (name, level, {k: (g[k], w[k]) for k in w if g.get(k) != w[k]})


# ---- the decode core on the host, under the sanitizers -----------------------------------------------------------------------
def write_job(path, job, table=None, sets=None, scans=None):
    table = job["table"] if table is None else table
    sets = job["sets"] if sets is None else sets
    scans = job["scans"] if scans is None else scans
    head = np.array([0x4A51534A, *job["geom"], int(job["transform"]), len(table), len(sets), len(scans), 0, 0, 0], dtype="<i4")
    with open(path, "wb") as f:
        f.write(head.tobytes() + np.ascontiguousarray(table, dtype="<i4").tobytes() + b"".join(sets) + np.asarray(scans, np.uint8).tobytes())


def read_out(path, job, n=None):
    n = len(job["table"]) if n is None else n
    w, h = job["geom"][:2]
    raw = open(path, "rb").read()
    assert len(raw) == 4 * n + n * w * h * 3
    return np.frombuffer(raw, dtype="<i4", count=n), np.frombuffer(raw, dtype=np.uint8, offset=4 * n).reshape(n, h, w, 3)


def huffman_codes(set_bytes, table):
    """{symbol: (length, code)} of table 0..3 (DC0, DC1, AC0, AC1) of a table set."""
    at = 512 + table * 272
    counts, symbols = set_bytes[at:at + 16], set_bytes[at + 16:at + 272]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (length, code)
            code += 1
            k += 1
        code <<= 1
    return out


def pack_bits(pieces):
    """[(length, value)] -> entropy-coded bytes: FF stuffed, the last byte padded with ones."""
    bits = "".join(format(v, f"0{n}b") for n, v in pieces if n)
    bits += "1" * (-len(bits) % 8)
    out = bytearray()
    for i in range(0, len(bits), 8):
        out.append(int(bits[i:i + 8], 2))
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out)


def damaged_jobs():
    """name -> (job, table, sets, scans, {slot: expected status}); every slot not listed must decode as in the good job."""
    out = {}
    with wsi.TiffSlide(fixture("ycc420")) as slide:
        job = slide.tile_job(0)
    third = job["table"].copy()
    third[0, 1] //= 3
    out["truncated_third"] = (job, third, None, None, {0: C["SQ_JPEG_TRUNCATED"]})
    last = job["table"].copy()
    last[2, 1] -= 1
    out["truncated_last_byte"] = (job, last, None, None, {2: C["SQ_JPEG_TRUNCATED"]})
    past = job["table"].copy()
    past[1, 0] = len(job["scans"]) - 2          # as a tile offset past the end of the file reaches the device: a range outside the buffer
    out["range_past_end"] = (job, past, None, None, {1: C["SQ_JPEG_BAD_RANGE"]})
    neg = job["table"].copy()
    neg[3, 0], neg[4, 1], neg[5, 2] = -8, 0, 7
    out["bad_rows"] = (job, neg, None, None, {3: C["SQ_JPEG_BAD_RANGE"], 4: C["SQ_JPEG_BAD_RANGE"], 5: C["SQ_JPEG_BAD_TABLE"]})
    over = bytearray(job["sets"][0])
    over[512 + 2 * 272] = 3                     # three codes of one bit in AC table 0: no prefix code
    out["oversubscribed_table"] = (job, None, [bytes(over)], None, {s: C["SQ_JPEG_BAD_TABLE"] for s in range(len(job["table"]))})
    # a run past coefficient 63, written by hand with the level's own tables: DC category 0, three ZRL, then run 15 / size 1
    dc, ac = huffman_codes(job["sets"][0], 0), huffman_codes(job["sets"][0], 2)
    run = pack_bits([dc[0], ac[0xF0], ac[0xF0], ac[0xF0], ac[0xF1], (1, 1)])
    scans = job["scans"].copy()
    a = int(job["table"][6, 0])
    assert len(run) <= job["table"][6, 1]
    scans[a:a + len(run)] = np.frombuffer(run, dtype=np.uint8)
    out["run_past_63"] = (job, None, None, scans, {6: C["SQ_JPEG_BAD_COEF"]})

    with wsi.TiffSlide(fixture("optimize")) as slide:
        opt = slide.tile_job(0)
    # the last code of the longest length of AC table 0 removed: an optimised table holds only symbols its tile uses
    sets = [bytearray(s) for s in opt["sets"]]
    victim = int(opt["table"][0, 2])
    at = 512 + 2 * 272
    longest = max(i for i in range(16) if sets[victim][at + i])
    sets[victim][at + longest] -= 1
    out["code_removed"] = (opt, None, [bytes(s) for s in sets], None, {0: C["SQ_JPEG_BAD_CODE"]})

    with wsi.TiffSlide(fixture("ycc422")) as slide:
        rst = slide.tile_job(0)
    scans = rst["scans"].copy()
    a, n = int(rst["table"][1, 0]), int(rst["table"][1, 1])
    seg = scans[a:a + n].tobytes()
    m = seg.index(b"\xff\xd0")
    scans[a + m + 1] = 0xD1
    out["restart_replaced"] = (rst, None, None, scans, {1: C["SQ_JPEG_BAD_RESTART"]})
    return out


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    """The stand-alone program built with the host compiler and the sanitizers, and a runner over a job directory."""
    return wc.build_hostcheck("jpegdec_hostcheck.cpp", tmp_path_factory.mktemp("hostcheck"), sanitize=True)


def test_host_build_of_the_core_equals_the_goldens_under_sanitizers(hostcheck, golden, tmp_path):
    jobs = {}
    for name in wc.CASES:
        with wsi.TiffSlide(fixture(name)) as slide:
            for level in range(slide.level_count):
                jobs[(name, level)] = slide.tile_job(level)
                write_job(tmp_path / f"{name}_L{level}.job", jobs[(name, level)])
    assert f"{len(jobs)} job(s), 0 failed" in hostcheck(tmp_path)
    for (name, level), job in jobs.items():
        status, rgb = read_out(tmp_path / f"{name}_L{level}.out", job)
        assert (status == 0).all(), (name, level, status)
        want = golden[f"{name}/L{level}/tiles"].transpose(0, 2, 3, 1)[job["tiles"]]
        assert np.array_equal(rgb, want), (name, level)


def test_damaged_streams_give_their_status_and_a_clean_sanitizer_run(hostcheck, golden, tmp_path):
    cases = damaged_jobs()
    good = {}
    for name, (job, table, sets, scans, expect) in cases.items():
        write_job(tmp_path / f"{name}.job", job, table, sets, scans)
        if id(job) not in good:
            good[id(job)] = f"good{len(good)}"
            write_job(tmp_path / f"{good[id(job)]}.job", job)
    hostcheck(tmp_path)
    for name, (job, table, sets, scans, expect) in cases.items():
        status, rgb = read_out(tmp_path / f"{name}.out", job)
        ok_status, ok_rgb = read_out(tmp_path / f"{good[id(job)]}.out", job)
        assert (ok_status == 0).all()
        for slot in range(len(status)):
            if slot in expect:
                assert status[slot] == expect[slot], (name, slot, status)
            else:                                   # every other tile of the batch is unaffected
                assert status[slot] == 0 and np.array_equal(rgb[slot], ok_rgb[slot]), (name, slot, status)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def parts_of(name):
    with wsi.TiffSlide(fixture(name)) as slide:
        offsets, counts = slide.tile_ranges(0)
        ifds, _ = wsi.read_ifds(slide._fd, slide._size)
        tables = bytes(ifds[slide._levels[0].index][347])
    raw = open(fixture(name), "rb").read()
    return tables, [raw[o:o + c] for o, c in zip(offsets, counts)]


def test_refusals_name_the_tag_and_its_value(tmp_path):
    tables, tiles = parts_of("single16")
    path = str(tmp_path / "bad.tif")

    def refuse(match, ifds=None, **kw):
        if ifds is not None:
            wc.write_tiff(path, ifds, **kw)
        with pytest.raises(wsi.WsiFormatError, match=match):
            wsi.TiffSlide(path)
    refuse("big-endian", [wc.level_ifd(16, 16, 16, tiles, 6, 2, tables)], byteorder=">")
    refuse(r"Compression = 33005 \(Aperio JPEG 2000", [wc.level_ifd(16, 16, 16, tiles, 6, 2, tables, compression=33005)])
    refuse(r"Compression = 5 \(LZW\)", [wc.level_ifd(16, 16, 16, tiles, 6, 2, tables, compression=5)])
    sof = tiles[0].index(b"\xff\xc0")
    progressive = tiles[0][:sof + 1] + b"\xc2" + tiles[0][sof + 2:]
    refuse(r"SOF2 \(0xc2, progressive\)", [wc.level_ifd(16, 16, 16, [progressive], 6, 2, tables)])
    arithmetic = tiles[0][:sof + 1] + b"\xc9" + tiles[0][sof + 2:]
    refuse(r"SOF9 \(0xc9, arithmetic-coded\)", [wc.level_ifd(16, 16, 16, [arithmetic], 6, 2, tables)])
    twelve = tiles[0][:sof + 4] + b"\x0c" + tiles[0][sof + 5:]
    refuse("sample precision 12", [wc.level_ifd(16, 16, 16, [twelve], 6, 2, tables)])
    refuse("TileWidth = 24", [wc.level_ifd(24, 24, 24, tiles, 6, 2, tables)])
    gray = tiles[0][:sof] + b"\xff\xc0" + struct.pack(">HBHHB", 11, 8, 16, 16, 1) + b"\x01\x11\x00" + tiles[0][sof + 19:]
    refuse("SOF0 with 1 components", [wc.level_ifd(16, 16, 16, [gray], 6, 2, tables)])
    one = wc.level_ifd(16, 16, 16, tiles, 6, 2, tables)
    one[277], one[258] = (3, 1), (3, [8])
    refuse("SamplesPerPixel = 1", [one])
    four = tiles[0][:sof + 11] + b"\x41" + tiles[0][sof + 12:]                   # luma sampling 4 x 1
    refuse(r"sampling factors \[\(4, 1\), \(1, 1\), \(1, 1\)\]", [wc.level_ifd(16, 16, 16, [four], 6, 2, tables)])
    refuse(r"SOF0 frame of 16 x 16 pixels in tiles of 32 x 32", [wc.level_ifd(32, 32, 32, tiles, 6, 2, tables)])
    refuse(r"TileByteCounts\[0\] = 0", [wc.level_ifd(16, 16, 16, [b""], 6, 2, tables)])
    # segments shorter than what the parser reads of them: the module's error, never an IndexError
    sos = tiles[0].index(b"\xff\xda")
    short_sof = tiles[0][:sof + 2] + struct.pack(">H", 10) + tiles[0][sof + 4:sof + 12] + tiles[0][sof + 19:]
    refuse("SOF0 of 3 components has a payload of 8 bytes", [wc.level_ifd(16, 16, 16, [short_sof], 6, 2, tables)])
    short_sos = tiles[0][:sos + 2] + struct.pack(">H", 6) + tiles[0][sos + 4:sos + 8] + tiles[0][sos + 14:]
    refuse("SOS of 3 components has a payload of 4 bytes", [wc.level_ifd(16, 16, 16, [short_sos], 6, 2, tables)])
    dri = tiles[0][:sof] + b"\xff\xdd" + struct.pack(">HB", 3, 0) + tiles[0][sof:]
    refuse("segment 0xdd at .* has a payload of 1 bytes", [wc.level_ifd(16, 16, 16, [dri], 6, 2, tables)])
    refuse("no tiled IFD", [wc.stripped_ifd(20, 12)])
    # a tile offset past the end of the file: named when that tile is read
    wc.write_tiff(path, [wc.level_ifd(16, 16, 16, tiles, 6, 2, tables)])
    raw = bytearray(open(path, "rb").read())
    with wsi.TiffSlide(path) as slide:
        offsets, _ = slide.tile_ranges(0)
    at = raw.index(struct.pack("<HHI", 324, 4, 1)) + 8
    assert struct.unpack_from("<I", raw, at)[0] == offsets[0]
    struct.pack_into("<I", raw, at, len(raw) + 100)
    open(path, "wb").write(raw)
    with wsi.TiffSlide(path) as slide:
        with pytest.raises(wsi.WsiFormatError, match=f"TileOffsets = {len(raw) + 100}"):
            slide.tile_job(0)


def test_reading_pixels_needs_the_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sequoia_pub_amd import _lib
    with wsi.TiffSlide(fixture("single16")) as slide:
        with pytest.raises(_lib.SequoiaHipError):
            slide.read_regions([(0, 0)], 0, (16, 16))
