"""Cases and helpers for the LZW and uncompressed tiled-TIFF reader (sequoia_pub_amd.wsi, csrc/tifflzw.hip, csrc/lzw_core.h).

``CASES`` lists the fixture files under tests/golden/tiffz/ (made by tests/golden/make_tiffz_golden.py: the tile streams are
Pillow's libtiff's, the container is written by ``wsi_cases.write_tiff``, and tiffz.npz holds every level as Pillow opens the
finished file).  ``lzw_encode`` is a small pure-Python TIFF LZW encoder (MSB first, libtiff's early change) with knobs libtiff's
own encoder does not have -- where it clears, whether it ends with EOI -- and ``lzw_decode`` the reference decoder; ``pillow_decode``
hands a stream to libtiff as a one-strip TIFF.  The job writer and reader speak tools/lzw_hostcheck.cpp's files."""
import io
import os

import numpy as np

import wsi_cases as wc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiffz")
CLEAR, EOI, FIRST = 256, 257, 258

# name -> levels [(width, height)], tile, compression (5 LZW, 1 none), predictor, content, bigtiff
CASES = {
    "flat16":   dict(levels=[(16, 16)], tile=16, compression=5, predictor=1, content="flat"),
    "flat16p":  dict(levels=[(16, 16)], tile=16, compression=5, predictor=2, content="flat"),
    "noise32":  dict(levels=[(32, 32)], tile=32, compression=5, predictor=1, content="rand"),
    "noise64":  dict(levels=[(64, 64)], tile=64, compression=5, predictor=1, content="rand"),
    "noise64p": dict(levels=[(64, 64)], tile=64, compression=5, predictor=2, content="rand"),
    "flat64":   dict(levels=[(64, 64)], tile=64, compression=5, predictor=1, content="flat"),
    "flat256":  dict(levels=[(256, 256)], tile=256, compression=5, predictor=1, content="flat"),
    "two64":    dict(levels=[(64, 64)], tile=64, compression=5, predictor=1, content="two"),
    "smooth":   dict(levels=[(150, 100), (75, 50)], tile=32, compression=5, predictor=2, content="smooth"),
    "big":      dict(levels=[(150, 100), (75, 50)], tile=32, compression=5, predictor=1, content="smooth", bigtiff=True),
    "raw16":    dict(levels=[(40, 24)], tile=16, compression=1, predictor=1, content="smooth"),
    "raw64":    dict(levels=[(70, 40)], tile=64, compression=1, predictor=1, content="smooth"),
}
# the synthetic slide of the pipeline tests: the smallest the patch filter admits (256-pixel regions)
PIPELINE = dict(levels=[(1024, 768), (128, 96)], tile=256, compression=5, predictor=2, content="tissue")


def spec_of(name):
    return PIPELINE if name == "pipeline" else CASES[name]


def fixture(name):
    return os.path.join(GOLDEN_DIR, f"{name}.tif")


def content_image(content, width, height, seed):
    """uint8 [height, width, 3]: wsi_cases.level_image's contents, and 'rand' (uniform noise) and 'two' (two colours at random)."""
    rng = np.random.RandomState(seed)
    if content == "rand":
        return rng.randint(0, 256, size=(height, width, 3)).astype(np.uint8)
    if content == "two":
        palette = np.array([[200, 110, 170], [236, 236, 236]], dtype=np.uint8)
        return palette[rng.randint(0, 2, size=(height, width))]
    return wc.level_image(content, width, height, seed)


def case_levels(name):
    """The level images of a case (uint8 [h, w, 3]): level i > 0 is level 0 decimated."""
    spec = spec_of(name)
    w0, h0 = spec["levels"][0]
    base = content_image(spec["content"], w0, h0, seed=sum(map(ord, name)) % 1000)
    out = [base]
    for w, h in spec["levels"][1:]:
        out.append(base[(np.arange(h) * h0) // h][:, (np.arange(w) * w0) // w].copy())
    return out


def level_tiles(img, tile):
    """The padded tiles [n, tile, tile, 3] of a level image, row-major."""
    h, w = img.shape[:2]
    return np.stack([wc.pad_tile(img, tx, ty, tile) for ty in range(-(-h // tile)) for tx in range(-(-w // tile))])


def tile_planes(tiles):
    """uint8 [n, th, tw, 3] chunky tiles -> [n, 3, th, tw], the planes the decoder writes."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(tiles), -1, -3))


# ---- predictor and LZW --------------------------------------------------------------------------------------------------------
def predict(tile, predictor):
    """The bytes of a chunky uint8 tile [h, w, 3] as they are compressed: Predictor 2 is the difference along each row, per
    channel, modulo 256."""
    tile = np.ascontiguousarray(tile, dtype=np.uint8)
    if predictor == 2:
        d = tile.copy()
        d[:, 1:] = tile[:, 1:] - tile[:, :-1]
        tile = d
    return tile.tobytes()


def unpredict(data, width, height, predictor):
    a = np.frombuffer(data, dtype=np.uint8).reshape(height, width, 3)
    return np.cumsum(a, axis=1, dtype=np.uint8) if predictor == 2 else a.copy()


def code_width(j):
    """Bits of the j-th code behind a Clear (libtiff's early change: 9 bits while the next free entry is below 511, ...)."""
    return 9 if j < 254 else 10 if j < 766 else 11 if j < 1790 else 12


class _Writer:
    def __init__(self):
        self.acc, self.n, self.out, self.j = 0, 0, bytearray(), 0

    def put(self, code, width=None):
        width = code_width(self.j) if width is None else width
        self.acc, self.n = (self.acc << width) | code, self.n + width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1
        self.j = 0 if code == CLEAR else self.j + 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xFF)
        return bytes(self.out)


def lzw_encode(data, clear_at=4094, clear_every=0, eoi=True, first_clear=True):
    """TIFF LZW of `data` (bytes).  ``clear_at``: the Clear code goes out when the entry of that number would be added (libtiff's
    encoder: 4094; None: never, entries past 4095 are simply not made); ``clear_every``: a Clear after every k codes as well;
    ``eoi``: end with the EOI code; ``first_clear``: start with the Clear code."""
    w = _Writer()
    if first_clear:
        w.put(CLEAR, 9)
    table, free, prefix, since = {}, FIRST, -1, 0
    for byte in data:
        if prefix < 0:
            prefix = byte
            continue
        key = (prefix << 8) | byte
        got = table.get(key)
        if got is not None:
            prefix = got
            continue
        w.put(prefix)
        since += 1
        prefix = byte
        if (clear_at is not None and free == clear_at) or (clear_every and since >= clear_every):
            w.put(CLEAR)
            table, free, since = {}, FIRST, 0
        elif free < 4096:
            table[key] = free
            free += 1
        else:
            free += 1                      # the decoder goes on counting entries it can never be asked for
    if prefix >= 0:
        w.put(prefix)
    if eoi:
        w.put(EOI)
    return w.done()


def lzw_decode(data, total):
    """The first `total` bytes a TIFF LZW stream decodes to, or a ValueError naming why it stops.  Entries are (position,
    length) ranges of the output, as in csrc/lzw_core.h; the segment limit is not restated here."""
    nbits = 8 * len(data)
    big = int.from_bytes(data, "big")

    def fetch(bit, width):
        return (big >> (nbits - bit - width)) & ((1 << width) - 1)
    if nbits < 9:
        raise ValueError("truncated")
    if fetch(0, 9) != CLEAR:
        raise ValueError("no clear")
    out, bit, j, entries = bytearray(), 9, 0, []
    while len(out) < total:
        width = code_width(j)
        if bit + width > nbits:
            raise ValueError("truncated")
        code = fetch(bit, width)
        bit += width
        if code == CLEAR:
            j, entries = 0, []
            continue
        if code == EOI:
            raise ValueError("eoi")
        at = len(out)
        if code < 256:
            out.append(code)
            entries.append((at, 1))
        else:
            i = code - FIRST
            if i >= j:
                raise ValueError("bad code")
            src, n = entries[i][0], entries[i][1] + 1
            for k in range(n):
                out.append(out[src + k])
            entries.append((at, n))
        j += 1
    return bytes(out[:total])


def strip_tiff(stream, width, height, compression=5, predictor=1):
    """The bytes of a one-strip TIFF around a tile's stream."""
    tags = {256: (4, width), 257: (4, height), 258: (3, [8, 8, 8]), 259: (3, compression), 262: (3, 2), 277: (3, 3), 278: (4, height),
            284: (3, 1), 273: [bytes(stream)]}
    if predictor != 1:
        tags[317] = (3, predictor)
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".tif") as f:
        wc.write_tiff(f.name, [tags])
        return open(f.name, "rb").read()


def has_libtiff():
    try:
        from PIL import features
        return bool(features.check("libtiff"))
    except ImportError:
        return False


def pillow_decode(stream, width, height, predictor=1):
    """uint8 [height, width, 3] as Pillow's libtiff decodes the stream, or None where it raises."""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(strip_tiff(stream, width, height, 5, predictor))) as im:
            return np.asarray(im.convert("RGB")).copy()
    except Exception:
        return None


# ---- encoder streams libtiff does not write -------------------------------------------------------------------------------------
# name -> (tile, content, predictor, encoder knobs); decoded by libtiff unless noted in the tests
VARIANTS = {
    "clear4094":   (64, "rand", 1, dict(clear_at=4094)),
    "clear4095":   (64, "rand", 1, dict(clear_at=4095)),
    "clear4096":   (64, "rand", 1, dict(clear_at=4096)),
    "never":       (64, "rand", 1, dict(clear_at=None)),
    "every100":    (32, "smooth", 2, dict(clear_every=100)),
    "every1":      (16, "smooth", 1, dict(clear_every=1)),
    "no_eoi":      (32, "smooth", 1, dict(eoi=False)),
    "never_short": (32, "rand", 1, dict(clear_at=None)),
}


def variant(name):
    """(stream, chunky tile uint8 [t, t, 3], predictor) of an encoder variant."""
    tile, content, predictor, knobs = VARIANTS[name]
    img = content_image(content, tile, tile, seed=sum(map(ord, name)) % 1000)
    return lzw_encode(predict(img, predictor), **knobs), img, predictor


def make_job(streams, tile_w, tile_h, compression=5, predictor=1):
    """A job like ``TiffSlide.tile_job``'s from stand-alone streams, slot i = stream i."""
    table = np.zeros((len(streams), 4), dtype=np.int32)
    at, parts = 0, []
    for i, s in enumerate(streams):
        table[i, :2] = (at, len(s))
        pad = -len(s) % 4
        parts.append(bytes(s) + b"\0" * pad)
        at += len(s) + pad
    scans = np.frombuffer(b"".join(parts) + b"\0" * (max((at + 15) & ~15, 16) - at), dtype=np.uint8).copy()
    return dict(codec="lzw" if compression == 5 else "raw", geom=(tile_w, tile_h, 1, 1), predictor=predictor, tiles=list(range(len(streams))),
                table=table, scans=scans)


# ---- tools/lzw_hostcheck.cpp's files ----------------------------------------------------------------------------------------------
def write_job(path, job, table=None, scans=None):
    table = job["table"] if table is None else table
    scans = job["scans"] if scans is None else scans
    head = np.array([0x575A4C53, job["geom"][0], job["geom"][1], len(table), len(scans), 5 if job["codec"] == "lzw" else 1, job["predictor"], 0],
                    dtype="<i4")
    with open(path, "wb") as f:
        f.write(head.tobytes() + np.ascontiguousarray(table, dtype="<i4").tobytes() + np.asarray(scans, np.uint8).tobytes())


def read_out(path, job, n=None):
    """(statuses int32 [n], planes uint8 [n, 3, h, w])"""
    n = len(job["table"]) if n is None else n
    w, h = job["geom"][:2]
    raw = open(path, "rb").read()
    assert len(raw) == 4 * n + n * w * h * 3
    return np.frombuffer(raw, dtype="<i4", count=n), np.frombuffer(raw, dtype=np.uint8, offset=4 * n).reshape(n, 3, h, w)


def build_hostcheck(directory, sanitize):
    """tools/lzw_hostcheck.cpp built with the host compiler into `directory`; returns a runner over a job directory that
    asserts a clean exit (and, with `sanitize`, a clean address / undefined-behaviour sanitizer run) and gives the output."""
    return wc.build_hostcheck("lzw_hostcheck.cpp", directory, sanitize)


# ---- the container ----------------------------------------------------------------------------------------------------------------
def level_ifd(width, height, tile, streams, compression, predictor, description=None):
    tags = wc.level_ifd(width, height, tile, streams, 2, 0, None, description, compression=compression)
    if predictor != 1:
        tags[317] = (3, predictor)
    return tags


def write_slide(path, levels, tile, compression, predictor, bigtiff=False, encode=None):
    """A tiled file of `levels` (uint8 [h, w, 3] images): every tile padded from the edge, predicted and encoded by `encode`
    (bytes -> stream, default ``lzw_encode``; uncompressed tiles are stored as they are)."""
    encode = lzw_encode if encode is None else encode
    ifds = []
    for img in levels:
        h, w = img.shape[:2]
        streams = [predict(t, predictor) if compression == 1 else encode(predict(t, predictor)) for t in level_tiles(img, tile)]
        ifds.append(level_ifd(w, h, tile, streams, compression, predictor))
    wc.write_tiff(path, ifds, bigtiff=bigtiff)


def damage(stream, kind):
    """A damaged copy of an encoder stream and the name of the status it must give."""
    s = bytearray(stream)
    if kind.startswith("cut"):
        return bytes(s[:int(kind[3:])]), "SQ_LZW_TRUNCATED"
    if kind == "bad_code":                  # the second code behind the Clear (bits 18..26) becomes 300: entry 258 is the next free one
        v = int.from_bytes(s[:4], "big")
        v = (v & ~(0x1FF << 5)) | (300 << 5)
        s[:4] = v.to_bytes(4, "big")
        return bytes(s), "SQ_LZW_BAD_CODE"
    if kind == "eoi_mid":                   # the third code behind the Clear (bits 27..35) becomes EOI
        v = int.from_bytes(s[:5], "big")
        v = (v & ~(0x1FF << 4)) | (EOI << 4)
        s[:5] = v.to_bytes(5, "big")
        return bytes(s), "SQ_LZW_EARLY_EOI"
    if kind == "no_clear":                  # the first nine bits become a literal
        s[0], s[1] = 0x20, s[1] & 0x7F
        return bytes(s), "SQ_LZW_NO_CLEAR"
    raise ValueError(kind)
