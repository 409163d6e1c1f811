"""The TIFF container of a slide (the package docstring has the rules): ``read_ifds``, the checks of a tiled IFD that every
compression shares (``check_samples``, ``Level``), the per-tile record ``TileInfo``, and ``Codec``, the base of the three codec
classes (jpeg.py, j2k.py, lzw.py) with what they share."""
import os
import struct
from typing import NamedTuple

import numpy as np

from . import WsiFormatError
from .._abi import CONSTANTS as _C

MAX_TILE = _C["SQ_JPEG_MAX_TILE"]
SCAN_BYTES_MAX = (1 << 31) - 64            # scan offsets in the tile table are int32

_TYPE = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d", 16: "Q", 17: "q", 18: "Q"}
TAG_NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation",
             266: "FillOrder", 270: "ImageDescription", 277: "SamplesPerPixel", 284: "PlanarConfiguration", 317: "Predictor", 322: "TileWidth",
             323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 338: "ExtraSamples", 347: "JPEGTables", 530: "YCbCrSubSampling"}


def read_ifds(fd, size):
    """Every IFD of a little-endian classic or BigTIFF file as a dict tag -> tuple of values (ASCII and UNDEFINED: bytes)."""
    head = os.pread(fd, 16, 0)
    if head[:2] == b"MM":
        raise WsiFormatError("byte order 'MM' (big-endian TIFF) is not supported: little-endian ('II') files only")
    if len(head) < 8 or head[:2] != b"II":
        raise WsiFormatError(f"not a TIFF file: it starts with {head[:4]!r}")
    magic = struct.unpack_from("<H", head, 2)[0]
    if magic == 42:
        big, offset = False, struct.unpack_from("<I", head, 4)[0]
    elif magic == 43:
        if len(head) < 16 or struct.unpack_from("<HH", head, 4) != (8, 0):
            raise WsiFormatError("BigTIFF header: offset size must be 8")
        big, offset = True, struct.unpack_from("<Q", head, 8)[0]
    else:
        raise WsiFormatError(f"TIFF magic {magic}: 42 (classic) or 43 (BigTIFF)")
    count_fmt, entry_fmt, inline = ("<Q", "<HHQ8s", 8) if big else ("<H", "<HHI4s", 4)
    entry_size, count_size = struct.calcsize(entry_fmt), struct.calcsize(count_fmt)
    ifds, seen = [], set()
    while offset:
        if offset in seen or offset + count_size > size:
            raise WsiFormatError(f"IFD offset {offset} is outside the file of {size} bytes or repeats")
        seen.add(offset)
        n = struct.unpack(count_fmt, os.pread(fd, count_size, offset))[0]
        raw = os.pread(fd, n * entry_size + inline, offset + count_size)
        if len(raw) < n * entry_size + inline:
            raise WsiFormatError(f"IFD at {offset} with {n} entries runs past the end of the file")
        tags = {}
        for i in range(n):
            tag, kind, count, value = struct.unpack_from(entry_fmt, raw, i * entry_size)
            if kind not in _TYPE:
                continue
            item = struct.calcsize("<" + _TYPE[kind])
            nbytes = item * count
            if nbytes <= inline:
                data = value[:nbytes]
            else:
                at = struct.unpack("<Q" if big else "<I", value)[0]
                if at + nbytes > size:
                    raise WsiFormatError(f"tag {tag} ({TAG_NAMES.get(tag, '?')}): {nbytes} bytes at offset {at} run past the end of the file")
                data = os.pread(fd, nbytes, at)
            if kind in (2, 7):
                tags[tag] = data
            elif kind in (5, 10):
                tags[tag] = tuple(np.frombuffer(data, dtype="<u4" if kind == 5 else "<i4").reshape(-1, 2).tolist())
            else:
                tags[tag] = np.frombuffer(data, dtype=np.dtype(_TYPE[kind]).newbyteorder("<"))
        ifds.append(tags)
        offset = struct.unpack("<Q" if big else "<I", raw[n * entry_size:n * entry_size + inline])[0]
    return ifds, big


def _one(tags, tag, default=None):
    v = tags.get(tag)
    if v is None:
        return default
    return int(v[0])


def need_tag(what, tags, tag, allowed, text):
    """The values of `tag` as ints, every one of them in `allowed`; else the refusal that names the tag, its value and `text`."""
    v = tags.get(tag)
    v = tuple(int(x) for x in v) if v is not None else None
    if v is None or any(x not in allowed for x in v):
        raise WsiFormatError(f"{what}: {TAG_NAMES[tag]} = {v if v is None or len(v) != 1 else v[0]}: {text}")
    return v


def check_samples(what, tags):
    """Three chunky samples of 8 bits: what every codec needs of BitsPerSample, SamplesPerPixel and PlanarConfiguration."""
    need_tag(what, tags, 258, (8,), "8 bits per sample only")
    if len(need_tag(what, tags, 277, (3,), "3 samples per pixel only")) != 1 or len(tags[258]) != 3:
        raise WsiFormatError(f"{what}: BitsPerSample = {tuple(int(x) for x in tags[258])}: three samples of 8 bits only")
    if _one(tags, 284, 1) != 1:
        raise WsiFormatError(f"{what}: PlanarConfiguration = {_one(tags, 284)}: 1 (chunky) only")


class Level:
    """The geometry, tile offsets and byte counts of one tiled IFD, and its ``codec``."""
    __slots__ = ("index", "width", "height", "tile_w", "tile_h", "tiles_x", "tiles_y", "offsets", "counts", "codec")

    def __init__(self, what, index, tags, codec):
        self.index, self.codec = index, codec
        self.width, self.height = _one(tags, 256, 0), _one(tags, 257, 0)
        self.tile_w, self.tile_h = _one(tags, 322, 0), _one(tags, 323, 0)
        if self.width < 1 or self.height < 1:
            raise WsiFormatError(f"{what}: ImageWidth = {self.width}, ImageLength = {self.height}")
        for tag, v in ((322, self.tile_w), (323, self.tile_h)):
            if v % 16 or not 16 <= v <= MAX_TILE:
                raise WsiFormatError(f"{what}: {TAG_NAMES[tag]} = {v}: a multiple of 16 in 16..{MAX_TILE} only")
        self.tiles_x, self.tiles_y = -(-self.width // self.tile_w), -(-self.height // self.tile_h)
        if 324 not in tags or 325 not in tags or len(tags[324]) != self.tiles_x * self.tiles_y or len(tags[325]) != len(tags[324]):
            raise WsiFormatError(f"{what}: TileOffsets / TileByteCounts must have {self.tiles_x * self.tiles_y} entries each")
        self.offsets, self.counts = tags[324].astype(np.int64), tags[325].astype(np.int64)
        if (self.counts == 0).any():
            t = int(np.flatnonzero(self.counts == 0)[0])
            raise WsiFormatError(f"{what}: TileByteCounts[{t}] = 0 (tile {t % self.tiles_x}, {t // self.tiles_x}): empty tiles are not supported")


class TileInfo(NamedTuple):
    """What the tile table and the upload need of one tile; ``restart`` and ``selectors`` are JPEG's, 0 elsewhere."""
    offset: int          # file offset of the bytes that go up: the scan, the packets, or the whole tile
    length: int
    tables: bytes        # table-set bytes (JPEG), parameter-set bytes (JPEG 2000), b"" where a tile needs none
    restart: int
    selectors: int


class Codec:
    """The format of one level's tiles.  A subclass checks the tags that are its own when it is built (and calls
    ``check_samples`` at its place among them: the first fault of an IFD is the one reported), and has ``name``, ``tile_words``
    and ``status_names``, ``_parse_tile``, ``chunk_tile_bytes``, ``decode`` and ``job_extras``.  Here: what the three share."""
    hs = vs = 1                          # the planes are written at full resolution
    transform = 0

    def __init__(self, slide, compression):
        self.slide, self.compression, self.lv, self.info = slide, compression, None, {}

    def attach(self, what, lv, tags):
        """The level's geometry, known once the container checks have passed; a subclass adds the checks that need it."""
        self.lv = lv

    @property
    def geom(self):
        return (self.lv.tile_w, self.lv.tile_h, self.hs, self.vs)

    def tile_info(self, t):
        """The ``TileInfo`` of tile t, parsed once."""
        got = self.info.get(t)
        if got is not None:
            return got
        lv, size = self.lv, self.slide._size
        what = f"IFD {lv.index} tile ({t % lv.tiles_x}, {t // lv.tiles_x})"
        off, count = int(lv.offsets[t]), int(lv.counts[t])
        if off < 0 or off + count > size:
            raise WsiFormatError(f"{what}: TileOffsets = {off} with TileByteCounts = {count} runs past the end of the file ({size} bytes)")
        got = self.info[t] = self._parse_tile(what, off, count)
        return got

    def table_row(self, at, info, set_index):
        """The tile-table row (``tile_words`` int32) of a slot whose bytes stand at `at` of the scans buffer."""
        return (at, info.length, set_index, 0)
