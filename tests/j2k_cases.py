"""Cases and helpers for the JPEG 2000 SVS reader (sequoia_pub_amd.wsi, csrc/j2kdec.hip, csrc/j2k_core.h).

``CASES`` lists the fixture files under tests/golden/j2k/ (made by tests/golden/make_j2k_golden.py with Pillow's OpenJPEG:
the .tif files, and j2k.npz with Pillow's decoded component planes of every tile stream).  The container is written by
``wsi_cases.write_tiff``.  ``encode_tile`` builds the raw codestream of one tile: Pillow's encoder directly, or the two
constructions Pillow does not expose -- 4:2:2 (three one-component CPRL streams joined behind one SIZ with sampling 1x1, 2x1,
2x1) and derived quantisation (QCD rewritten to its first step, or a QCC of that kind added for one component).  The job
writer and reader speak tools/j2k_hostcheck.cpp's files; ``compose`` is the colour step of sq_jpeg_compose_regions in numpy."""
import io
import os
import struct

import numpy as np

import wsi_cases as wc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "j2k")
APERIO = "Aperio Image Library v11.2.1\r\n{w}x{h} [0,0 {w}x{h}] ({tw}x{th}) J2K/KDU Q=30|AppMag = 20|MPP = 0.5021|Filename = synthetic"

LOSSY = dict(irreversible=True, quality_mode="dB", quality_layers=[38])
# name -> levels, tile (w, h), compression, Pillow options, and: s422 (the 4:2:2 construction), derived ('qcd' / 'qcc'),
# exact (every byte Pillow's: reversible with every pass present), content, bigtiff
CASES = {
    "aperio05":  dict(levels=[(400, 260), (200, 130)], tile=(240, 240), compression=33005, opts=dict(LOSSY, num_resolutions=6, mct=1, codeblock_size=(64, 64), progression="LRCP")),
    "aperio03":  dict(levels=[(400, 260), (200, 130)], tile=(240, 240), compression=33003, s422=True, opts=dict(LOSSY, num_resolutions=6, codeblock_size=(64, 64))),
    "odd":       dict(levels=[(48, 80)], tile=(48, 80), compression=33005, opts=dict(LOSSY, num_resolutions=6, mct=1)),
    # 80 x 48, not 48 x 80: OpenJPEG's encoder refuses 5 levels on a 24-pixel-wide chroma plane (chroma here 40 -> 20 -> 10 -> 5 -> 3 -> 2)
    "odd422":    dict(levels=[(80, 48)], tile=(80, 48), compression=33003, s422=True, opts=dict(LOSSY, num_resolutions=6)),
    "single16":  dict(levels=[(16, 16)], tile=(16, 16), compression=33005, opts=dict(LOSSY, num_resolutions=5, mct=1)),
    "levels0":   dict(levels=[(50, 40)], tile=(32, 32), compression=33005, opts=dict(LOSSY, num_resolutions=1, mct=1)),
    "cb32":      dict(levels=[(100, 70)], tile=(64, 64), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, codeblock_size=(32, 32))),
    "cb16x64":   dict(levels=[(100, 70)], tile=(64, 64), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, codeblock_size=(16, 64))),
    "layers3":   dict(levels=[(100, 70)], tile=(64, 64), compression=33005, opts=dict(irreversible=True, quality_mode="dB", quality_layers=[30, 35, 40], num_resolutions=4, mct=1, progression="RLCP")),
    "precinct":  dict(levels=[(128, 128)], tile=(128, 128), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, precinct_size=(64, 64), codeblock_size=(32, 32), progression="LRCP")),
    "rpcl":      dict(levels=[(64, 64)], tile=(64, 64), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, progression="RPCL")),
    "pcrl":      dict(levels=[(64, 64)], tile=(64, 64), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, progression="PCRL")),
    "plt":       dict(levels=[(64, 64)], tile=(64, 64), compression=33005, opts=dict(LOSSY, num_resolutions=4, mct=1, plt=True)),
    "rct":       dict(levels=[(50, 40)], tile=(32, 32), compression=33005, exact=True, opts=dict(irreversible=False, num_resolutions=4, mct=1)),
    "plain53":   dict(levels=[(50, 40)], tile=(32, 32), compression=33005, exact=True, opts=dict(irreversible=False, num_resolutions=4, mct=0)),
    "cut53":     dict(levels=[(64, 64)], tile=(64, 64), compression=33005, opts=dict(irreversible=False, quality_mode="dB", quality_layers=[36], num_resolutions=4, mct=1)),
    "derived":   dict(levels=[(64, 64)], tile=(64, 64), compression=33005, derived="qcd", opts=dict(LOSSY, num_resolutions=4, mct=1)),
    "qcc":       dict(levels=[(64, 64)], tile=(64, 64), compression=33005, derived="qcc", opts=dict(LOSSY, num_resolutions=4, mct=0)),
    "big":       dict(levels=[(100, 70), (50, 35)], tile=(64, 64), compression=33005, bigtiff=True, opts=dict(LOSSY, num_resolutions=4, mct=1)),
    "noise":     dict(levels=[(32, 32)], tile=(32, 32), compression=33005, exact=True, content="noise", opts=dict(irreversible=False, num_resolutions=3, mct=1)),
}
# the synthetic slide of the pipeline tests: the smallest the patch filter admits (256-pixel regions); lossless, so its pixels
# are the array the other route is given
PIPELINE = dict(levels=[(1024, 768), (128, 96)], tile=(256, 256), compression=33005, exact=True, content="tissue",
                opts=dict(irreversible=False, num_resolutions=6, mct=1))


def spec_of(name):
    return PIPELINE if name == "pipeline" else CASES[name]


def fixture(name):
    return os.path.join(GOLDEN_DIR, f"{name}.tif")


def case_levels(name):
    """The level images of a case (uint8 [h, w, 3]): level i > 0 is level 0 decimated."""
    spec = spec_of(name)
    w0, h0 = spec["levels"][0]
    content = spec.get("content", "smooth")
    if content == "noise":
        base = np.random.RandomState(7).randint(0, 256, size=(h0, w0, 3)).astype(np.uint8)
    else:
        base = wc.level_image(content, w0, h0, seed=sum(map(ord, name)) % 1000)
    out = [base]
    for w, h in spec["levels"][1:]:
        out.append(base[(np.arange(h) * h0) // h][:, (np.arange(w) * w0) // w].copy())
    return out


def pad_tile(img, tx, ty, tile):
    h, w = img.shape[:2]
    ys = np.minimum(np.arange(ty * tile[1], (ty + 1) * tile[1]), h - 1)
    xs = np.minimum(np.arange(tx * tile[0], (tx + 1) * tile[0]), w - 1)
    return img[ys][:, xs]


# ---- codestream surgery ---------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, start, end)] of the header segments up to SOD (start at the ff, end behind the payload), SOD's own position last."""
    out, pos = [], 2
    while data[pos + 1] != 0x93:
        length = (data[pos + 2] << 8) | data[pos + 3]
        out.append((data[pos + 1], pos, pos + 2 + length))
        pos += 2 + length
    out.append((0x93, pos, pos + 2))
    return out


def segment(data, marker):
    for m, a, b in segments(data):
        if m == marker:
            return a, b
    raise KeyError(hex(marker))


def with_psot(data):
    """`data` with the Psot of its one SOT set to what now lies between SOT and EOC."""
    a, _ = segment(data, 0x90)
    end = len(data) - 2 if data[-2:] == b"\xff\xd9" else len(data)
    return data[:a + 6] + struct.pack(">I", end - a) + data[a + 10:]


def derived_qcd(data):
    """The QCD of `data` from expounded to derived: the first step size only."""
    a, b = segment(data, 0x5C)
    sqcd = data[a + 4]
    assert sqcd & 31 == 2
    seg = b"\xff\x5c" + struct.pack(">HB", 5, (sqcd & 0xE0) | 1) + data[a + 5:a + 7]
    return with_psot(data[:a] + seg + data[b:])


def derived_qcc(data, component=1):
    """A QCC for one component behind the QCD of `data`: the QCD's guard bits, derived from its first step size."""
    a, b = segment(data, 0x5C)
    sqcd = data[a + 4]
    assert sqcd & 31 == 2
    seg = b"\xff\x5d" + struct.pack(">HBB", 6, component, (sqcd & 0xE0) | 1) + data[a + 5:a + 7]
    return with_psot(data[:b] + seg + data[b:])


def join_422(y, cb, cr):
    """Three one-component CPRL streams (Y at W x H, Cb and Cr at W/2 x H, equal options) as one stream with SIZ sampling
    1x1, 2x1, 2x1: the main header of Y with three components, then the three tile bodies behind one SOT."""
    parts = []
    for s in (y, cb, cr):
        sod = segments(s)[-1][1]
        end = len(s) - 2 if s[-2:] == b"\xff\xd9" else len(s)
        parts.append(s[sod + 2:end])
    (ya, yb), (ca, cb_) = segment(y, 0x52), segment(cb, 0x52)
    assert y[ya + 4:yb] == cb[ca + 4:cb_] and y[slice(*segment(y, 0x5C))] == cb[slice(*segment(cb, 0x5C))]       # COD, QCD payloads equal
    assert y[ya + 5] == 4                                                                                      # CPRL
    a, b = segment(y, 0x51)
    siz = bytearray(y[a:b])
    assert siz[4 + 34:4 + 36] == b"\x00\x01"
    siz[4 + 34:4 + 36] = b"\x00\x03"
    siz += bytes([7, 2, 1, 7, 2, 1])
    siz[2:4] = struct.pack(">H", len(siz) - 2)
    out = y[:a] + bytes(siz) + y[b:segments(y)[-1][1] + 2] + b"".join(parts) + b"\xff\xd9"
    return with_psot(out)


def pillow_encode(arr, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(buf, "JPEG2000", no_jp2=True, **opts)
    return buf.getvalue()


def pillow_decode(stream):
    """uint8 [3, h, w] (or [1, h, w]) as Pillow's OpenJPEG decodes a raw codestream: the components as stored or, with the
    stream's component transform on, RGB."""
    from PIL import Image
    im = np.asarray(Image.open(io.BytesIO(stream)))
    return np.ascontiguousarray(im[None] if im.ndim == 2 else im.transpose(2, 0, 1))


def rgb_to_ycc(rgb):
    """JFIF YCbCr of an RGB tile, what a 33003 file's encoder stores."""
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    return np.clip(np.rint(np.stack([y, 128 + (b - y) * 0.564, 128 + (r - y) * 0.713], -1)), 0, 255).astype(np.uint8)


def encode_tile(rgb, spec):
    """(stream, witness planes uint8 [3, h, w]) of one tile."""
    opts = spec["opts"]
    if spec.get("s422"):
        ycc = rgb_to_ycc(rgb)
        cb, cr = (ycc[:, :, i].reshape(ycc.shape[0], -1, 2).mean(-1).round().astype(np.uint8) for i in (1, 2))
        o = dict(opts, progression="CPRL")
        streams = [pillow_encode(p, **o) for p in (ycc[:, :, 0], cb, cr)]
        planes = [pillow_decode(s)[0] for s in streams]
        return join_422(*streams), np.stack([planes[0], np.repeat(planes[1], 2, axis=1), np.repeat(planes[2], 2, axis=1)])
    data = pillow_encode(rgb_to_ycc(rgb) if spec["compression"] == 33003 else rgb, **opts)
    if spec.get("derived") == "qcd":
        data = derived_qcd(data)
    elif spec.get("derived") == "qcc":
        data = derived_qcc(data)
    return data, pillow_decode(data)


def compose(planes, transform):
    """uint8 [..., 3, h, w] component planes -> RGB [..., h, w, 3] as sq_jpeg_compose_regions gives it: libjpeg's fixed-point
    YCbCr -> RGB when `transform`, else the planes as stored."""
    p = np.moveaxis(planes.astype(np.int64), -3, -1)
    if not transform:
        return p.astype(np.uint8)
    y, cb, cr = p[..., 0], p[..., 1] - 128, p[..., 2] - 128
    rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)]
    return np.clip(np.stack(rgb, -1), 0, 255).astype(np.uint8)


def assemble(tiles, width, height, tile):
    """Tiles [n, th, tw, 3] row-major -> the level image, cropped."""
    tx = -(-width // tile[0])
    out = np.zeros((height, width, 3), dtype=np.uint8)
    for t, img in enumerate(tiles):
        y, x = (t // tx) * tile[1], (t % tx) * tile[0]
        out[y:y + tile[1], x:x + tile[0]] = img[:height - y, :width - x]
    return out


def level_witness(golden, name, level):
    """The RGB level image [h, w, 3] of a case from the goldens' tile planes."""
    spec = spec_of(name)
    w, h = spec["levels"][level]
    return assemble(compose(golden[f"{name}/L{level}/tiles"], spec["compression"] == 33003), w, h, spec["tile"])


def check_parity(got, want, exact, what):
    """The parity rule of the suite: `exact` cases equal Pillow byte for byte; the others are within 1 grey level with at most
    1 % of the bytes different.  Returns (share of different bytes, largest difference)."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share, worst = float((d > 0).mean()), int(d.max())
    print(f"{what}: {share:.6f} of the bytes differ, by at most {worst}")
    if exact:
        assert worst == 0, (what, share, worst)
    else:
        assert worst <= 1 and share <= 0.01, (what, share, worst)
    return share, worst


# ---- tools/j2k_hostcheck.cpp's files -----------------------------------------------------------------------------------------
def write_job(path, job, table=None, sets=None, scans=None):
    table = job["table"] if table is None else table
    sets = job["sets"] if sets is None else sets
    scans = job["scans"] if scans is None else scans
    head = np.array([0x4B324A4A, job["geom"][0], job["geom"][1], len(table), len(sets), len(scans), *job["caps"], 0, 0, 0], dtype="<i4")
    with open(path, "wb") as f:
        f.write(head.tobytes() + np.ascontiguousarray(table, dtype="<i4").tobytes() + b"".join(sets) + np.asarray(scans, np.uint8).tobytes())


def read_out(path, job, n=None):
    """(statuses int32 [n], planes uint8 [n, 3, h, w])"""
    n = len(job["table"]) if n is None else n
    w, h = job["geom"][:2]
    raw = open(path, "rb").read()
    assert len(raw) == 4 * n + n * w * h * 3
    return np.frombuffer(raw, dtype="<i4", count=n), np.frombuffer(raw, dtype=np.uint8, offset=4 * n).reshape(n, 3, h, w)


def build_hostcheck(directory, sanitize):
    """tools/j2k_hostcheck.cpp built with the host compiler into `directory`; returns a runner over a job directory that
    asserts a clean exit (and, with `sanitize`, a clean address / undefined-behaviour sanitizer run) and gives the output."""
    return wc.build_hostcheck("j2k_hostcheck.cpp", directory, sanitize, extra_flags=("-ffp-contract=off",))


# ---- damaged streams --------------------------------------------------------------------------------------------------------
def pack_header_bits(bits):
    """A string of '0' / '1' as packet-header bytes: the byte after an ff carries 7 bits, the last byte is padded with zeros."""
    out, i, after_ff = bytearray(), 0, False
    while i < len(bits):
        take = 7 if after_ff else 8
        chunk = bits[i:i + take].ljust(take, "0")
        out.append(int(chunk, 2))
        after_ff = out[-1] == 0xFF
        i += take
    if after_ff:
        out.append(0)
    return bytes(out)


# first packet of a tile whose first precinct-band has one code-block: present, included (tag tree bit), no missing bit-planes
# (tag tree bit), one pass ('0'), then Lblock raised by 13 to 16 and a length of sixteen ones: 65535 bytes
LENGTH_PAST_STREAM = pack_header_bits("1" + "1" + "1" + "0" + "1" * 13 + "0" + "1" * 16)


def damage_file(src, dst):
    """The 'rct' fixture (2 x 2 tiles, lossless) with tile (1, 0) cut one byte short (inside its last packet's body) and the
    first packet header of tile (0, 1) overwritten with LENGTH_PAST_STREAM.  Returns {tile number: expected status name}."""
    from sequoia_pub_amd import wsi
    raw = bytearray(open(src, "rb").read())
    with wsi.TiffSlide(src) as slide:
        offsets, counts = slide.tile_ranges(0)
        body = slide._tile_info(slide._levels[0], 2)[0]
    at = raw.index(np.asarray(counts, dtype="<u4").tobytes())
    eoc = 2 if raw[int(offsets[1]) + int(counts[1]) - 2:int(offsets[1]) + int(counts[1])] == b"\xff\xd9" else 0
    struct.pack_into("<I", raw, at + 4 * 1, int(counts[1]) - eoc - 1)
    raw[body:body + len(LENGTH_PAST_STREAM)] = LENGTH_PAST_STREAM
    with open(dst, "wb") as f:
        f.write(raw)
    return {1: "SQ_J2K_TRUNCATED_BODY", 2: "SQ_J2K_BAD_LENGTH"}
