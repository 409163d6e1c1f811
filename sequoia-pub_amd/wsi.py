"""JPEG-, JPEG 2000-, LZW-tiled and uncompressed tiled TIFF and Aperio SVS slides without openslide: ``TiffSlide`` is the drop-in for ``openslide.OpenSlide`` over
the interface subset this package uses (``dimensions``, ``level_count``, ``level_dimensions``, ``level_downsamples``,
``properties``, ``read_region``, ``close``), replacing the region reads of pre_processing/patch_gen_hdf5.py:45,108 and
spatial_vis/visualize.py:58-66,173.  The container is parsed here in Python (``struct`` + ``os.pread``, no GPU needed); the
tiles are decoded by the library on the device (``sq_jpeg_decode_tiles``, ``sq_jpeg_compose_regions``: csrc/jpegdec.hip), every
byte libjpeg's, and ``read_regions`` hands a whole batch of regions over as one uint8 [k, h, w, 4] device tensor in the layout
the patch filter, the slide mask, the resize and the pack kernels read -- no pixel is ever on the host.  Reading pixels needs
the GPU: there is no CPU fallback.

Accepted: classic TIFF (magic 42) and BigTIFF (43), little-endian; a level is an IFD with TileWidth / TileLength, levels
ordered by decreasing width; stripped IFDs (thumbnail, label, macro of an SVS) are skipped as OpenSlide skips them.  A tiled
IFD of compression 7 (JPEG; 33003 / 33005 and 5 / 1 are described below) must have 8 bits per sample, 3 samples per pixel, planar configuration 1, photometric 2 (RGB) or 6
(YCbCr), tile extents that are multiples of 16 in 16..1024, and baseline frames of exactly the tile extent with luma sampling
1x1, 2x1 or 2x2 over chroma 1x1.  Everything else -- big-endian files, any other compression (34712 among them),
progressive, arithmetic or 12-bit frames, 1 or 4 components, other samplings, a tile with byte count 0 -- is refused with a
``WsiFormatError`` that names the tag or marker and its value.  The TIFF photometric tag decides the colour transform as libtiff
does (6: YCbCr -> RGB, 2: components as stored); JFIF and Adobe markers of the stream are ignored.

JPEG 2000 levels (compression 33003 / 33005, Aperio's ``J2K/KDU``; a level is one codec): a tile is one raw codestream (SOC ... EOC, no
JP2 boxes), decoded by ``sq_j2k_decode_tiles`` (csrc/j2kdec.hip) into the planes ``sq_jpeg_compose_regions`` reads.  33003: the
components are YCbCr and go through libjpeg's fixed-point YCbCr -> RGB; 33005: RGB as stored; the photometric tag is not consulted
(believed to be what OpenSlide does; it is not installed, and no digit-for-digit claim against it is made).  ``parse_j2k`` walks
SIZ, COD, COC, QCD, QCC, SOT up to SOD (COM, PLT skipped) and accepts: 3 components of 8 bits unsigned, offsets 0, one tile of the
TIFF tile's extent in one tile-part, sampling 1x1 everywhere or 1x1, 2x1, 2x1 (4:2:2, chroma replicated); 0..8 levels, 5/3 or 9/7,
the component transform on (1x1 sampling only) or off, 1..32 layers, code-blocks of 4..64, code-block style 0, quantisation styles
none, derived and expounded (QCC per component; a COC must repeat the COD), LRCP and RLCP with any precincts (at most 256 per
resolution), RPCL / PCRL / CPRL with one precinct per resolution.  Refused by name: any code-block style bit, SOP / EPH, POC, RGN,
PPM / PPT, TLM, several tiles or tile-parts, other depths and component counts, code-blocks above 64, positional progressions with
several precincts.  Python touches marker segments only: packet headers are parsed on the device.  Against Pillow's OpenJPEG the
bytes are equal for reversible streams with every pass present and within 1 grey level (about 1 byte in 1000) otherwise.

LZW and uncompressed levels (compression 5 / 1: the lossless pyramids libvips, QuPath, Bio-Formats and tiffcp write; a level is one
codec): a tile is chunky RGB of 8 bits, decoded by ``sq_lzw_decode_tiles`` (csrc/tifflzw.hip, csrc/lzw_core.h) into the same planes,
every byte libtiff's.  Accepted: photometric 2 (RGB), three samples of 8 bits, planar configuration 1, FillOrder absent or 1,
Predictor absent, 1 or 2 (horizontal differencing, undone on the device), the tile extents above; LZW streams MSB first with
libtiff's early change, opening with the Clear code.  Refused by name: Predictor 3, ExtraSamples or four samples (RGBA), FillOrder
2, any other photometric, an uncompressed tile whose byte count is not tile width x height x 3, old-style LZW (LSB first, no
Clear at the start); deflate (8, 32946) and every other compression.  A stream that overruns the code table without a Clear is
refused where libtiff refuses it, when the tile is read (``TileDecodeError``).

Region semantics: ``location`` is in level-0 pixels, the level origin is ``(int(x / downsample), int(y / downsample))`` with
``downsample = level0_width / level_width``; pixels outside the level are (0, 0, 0, 0), inside alpha is 255.  At level 0 and
for reads from (0, 0) -- the only reads this package makes -- that is what OpenSlide returns.  OpenSlide interpolates a
fractional origin at higher levels; this reader does not."""
import os
import struct

import numpy as np

from . import _lib
from ._abi import CONSTANTS as _C

TILE_WORDS, TABLE_SET_BYTES, MAX_TILE = _C["SQ_JPEG_TILE_WORDS"], _C["SQ_JPEG_TABLE_SET_BYTES"], _C["SQ_JPEG_MAX_TILE"]
STATUS_NAMES = {_C["SQ_JPEG_BAD_TABLE"]: "a Huffman table that is no prefix code or a missing table set",
                _C["SQ_JPEG_BAD_RANGE"]: "a scan range outside the uploaded bytes",
                _C["SQ_JPEG_TRUNCATED"]: "the scan ends before its last MCU",
                _C["SQ_JPEG_BAD_CODE"]: "a code that matches no Huffman table entry",
                _C["SQ_JPEG_BAD_COEF"]: "a zero run past coefficient 63",
                _C["SQ_JPEG_BAD_RESTART"]: "a missing or wrong restart marker"}
J2K_TILE_WORDS = _C["SQ_J2K_TILE_WORDS"]
J2K_STATUS_NAMES = {_C["SQ_J2K_BAD_PARAM"]: "a parameter-set field out of range or a missing parameter set",
                    _C["SQ_J2K_BAD_RANGE"]: "a packet range outside the uploaded bytes",
                    _C["SQ_J2K_TRUNCATED_HEADER"]: "a packet header runs past the end of the tile's bytes",
                    _C["SQ_J2K_BAD_LENGTH"]: "a pass count, bit-plane count or length that does not fit the code-block or the stream",
                    _C["SQ_J2K_TRUNCATED_BODY"]: "the code-block bytes of a packet run past the end of the tile's bytes"}
LZW_TILE_WORDS = _C["SQ_LZW_TILE_WORDS"]
LZW_STATUS_NAMES = {_C["SQ_LZW_BAD_RANGE"]: "a tile range outside the uploaded bytes",
                    _C["SQ_LZW_TRUNCATED"]: "the tile's bytes end before the tile is full",
                    _C["SQ_LZW_BAD_CODE"]: "an LZW code above the next free table entry",
                    _C["SQ_LZW_NO_CLEAR"]: "an LZW stream that does not start with the Clear code",
                    _C["SQ_LZW_TABLE_FULL"]: "an LZW stream that overruns the code table without a Clear code",
                    _C["SQ_LZW_EARLY_EOI"]: "the LZW end-of-information code before the tile is full"}
LZW_COMPRESSIONS = {5: "LZW", 1: "uncompressed"}
LZW_MODE = _C["SQ_LZW_MODE_WAVE"]         # SQ_LZW_MODE_WAVE: a wave per tile; SQ_LZW_MODE_LANE: a lane per tile, the serial reference
SCAN_BYTES_MAX = (1 << 31) - 64            # scan offsets in the tile table are int32
DEFAULT_WORKSPACE_BUDGET = 1 << 30        # bytes of device workspace (planes, coefficients, uploaded scans) per chunk of a batch

_TYPE = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 6: "b", 7: "B", 8: "h", 9: "i", 10: "ii", 11: "f", 12: "d", 16: "Q", 17: "q", 18: "Q"}
_TAG_NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation",
              266: "FillOrder", 270: "ImageDescription", 277: "SamplesPerPixel", 284: "PlanarConfiguration", 317: "Predictor", 322: "TileWidth",
              323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 338: "ExtraSamples", 347: "JPEGTables", 530: "YCbCrSubSampling"}


class WsiFormatError(ValueError):
    """The file is not one this reader takes; the message names the tag or marker and its value."""


class TileDecodeError(RuntimeError):
    """Tiles of a batch did not decode.  ``tiles``: [(level, tile_x, tile_y, status)]; ``regions``: the batch's device tensor,
    every tile but the failing ones decoded; ``first_failed_region``: the first region of the batch that lies on one of them."""

    def __init__(self, message, tiles, regions, first_failed_region):
        super().__init__(message)
        self.tiles, self.regions, self.first_failed_region = tiles, regions, first_failed_region


# ---- TIFF container ---------------------------------------------------------------------------------------------------
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
                    raise WsiFormatError(f"tag {tag} ({_TAG_NAMES.get(tag, '?')}): {nbytes} bytes at offset {at} run past the end of the file")
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


# ---- JPEG headers -----------------------------------------------------------------------------------------------------
class JpegHeader:
    """Tables and frame of one (possibly abbreviated) stream: quant {id: uint16[64] zigzag}, huff {(class, id): (counts, symbols)},
    frame (marker, precision, height, width, [(id, h, v, tq)]), scan [(component id, td, ta)], restart interval, and the byte
    range [scan_start, scan_end) of the entropy-coded segment."""
    __slots__ = ("quant", "huff", "frame", "scan", "restart", "scan_start", "scan_end", "own_tables")

    def __init__(self):
        self.quant, self.huff, self.frame, self.scan = {}, {}, None, None
        self.restart, self.scan_start, self.scan_end, self.own_tables = 0, None, None, False


def parse_jpeg(data, base=None, what="JPEG stream"):
    """Walk the marker segments of `data` (bytes).  `base`: a JpegHeader whose tables this stream starts from (JPEGTables)."""
    h = JpegHeader()
    if base is not None:
        h.quant, h.huff, h.restart = dict(base.quant), dict(base.huff), base.restart
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise WsiFormatError(f"{what}: no SOI marker at its start")
    pos = 2
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            raise WsiFormatError(f"{what}: byte {data[pos]:#x} at {pos} where a marker was expected")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0xD9:
            break
        length = (data[pos + 2] << 8) | data[pos + 3]
        seg, end = pos + 4, pos + 2 + length
        if length < 2 or end > n:
            raise WsiFormatError(f"{what}: segment {m:#x} at {pos} of length {length} runs past the end")
        need = {0xDD: 2, 0xDA: 1}.get(m, 0)                     # payload bytes indexed below (SOF0 and SOS check theirs as they go)
        if end - seg < need:
            raise WsiFormatError(f"{what}: segment {m:#x} at {pos} has a payload of {end - seg} bytes, at least {need} are needed")
        if m == 0xDB:
            h.own_tables = True
            while seg < end:
                pq, tq = data[seg] >> 4, data[seg] & 15
                if pq not in (0, 1) or tq > 3 or seg + 1 + 64 * (pq + 1) > end:
                    raise WsiFormatError(f"{what}: DQT with precision {pq}, table {tq}")
                vals = np.frombuffer(data, dtype=">u2" if pq else np.uint8, count=64, offset=seg + 1).astype(np.uint16)
                h.quant[tq] = vals
                seg += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            h.own_tables = True
            while seg < end:
                tc, th = data[seg] >> 4, data[seg] & 15
                counts = bytes(data[seg + 1:seg + 17])
                total = sum(counts)
                if tc > 1 or th > 1 or len(counts) < 16 or total > 256 or seg + 17 + total > end:
                    raise WsiFormatError(f"{what}: DHT class {tc}, table {th} with {total} symbols: baseline takes classes 0..1, tables 0..1, "
                                         f"at most 256 symbols")
                h.huff[(tc, th)] = (counts, bytes(data[seg + 17:seg + 17 + total]))
                seg += 17 + total
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if m != 0xC0:
                kind = {0xC1: "extended sequential", 0xC2: "progressive", 0xC9: "arithmetic-coded"}.get(m, "not baseline")
                raise WsiFormatError(f"{what}: frame marker SOF{m - 0xC0} ({m:#x}, {kind}) is not supported: baseline (SOF0) only")
            if end - seg < 6:
                raise WsiFormatError(f"{what}: segment {m:#x} at {pos} has a payload of {end - seg} bytes, at least 6 are needed")
            precision, height, width, nc = data[seg], (data[seg + 1] << 8) | data[seg + 2], (data[seg + 3] << 8) | data[seg + 4], data[seg + 5]
            if precision != 8:
                raise WsiFormatError(f"{what}: SOF0 sample precision {precision}: 8 bits only")
            if nc != 3:
                raise WsiFormatError(f"{what}: SOF0 with {nc} components: 3 only")
            if end - seg < 15:
                raise WsiFormatError(f"{what}: SOF0 of 3 components has a payload of {end - seg} bytes, 15 are needed")
            comps = [(data[seg + 6 + 3 * i], data[seg + 7 + 3 * i] >> 4, data[seg + 7 + 3 * i] & 15, data[seg + 8 + 3 * i]) for i in range(3)]
            h.frame = (m, precision, height, width, comps)
        elif m == 0xDD:
            h.restart = (data[seg] << 8) | data[seg + 1]
        elif m == 0xDA:
            ns = data[seg]
            if ns != 3 or h.frame is None:
                raise WsiFormatError(f"{what}: SOS with {ns} components: one interleaved scan of 3 only")
            if end - seg < 10:
                raise WsiFormatError(f"{what}: SOS of 3 components has a payload of {end - seg} bytes, 10 are needed")
            h.scan = [(data[seg + 1 + 2 * i], data[seg + 2 + 2 * i] >> 4, data[seg + 2 + 2 * i] & 15) for i in range(3)]
            h.scan_start = end
            tail = data.rfind(b"\xff\xd9", end) if isinstance(data, (bytes, bytearray)) else -1
            h.scan_end = tail if tail >= 0 else n
            return h
        pos = end
    return h


def _sampling(frame, what):
    comps = frame[4]
    (hs, vs), chroma = (comps[0][1], comps[0][2]), [(c[1], c[2]) for c in comps[1:]]
    if chroma != [(1, 1), (1, 1)] or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
        raise WsiFormatError(f"{what}: SOF0 sampling factors {[(c[1], c[2]) for c in comps]}: luma 1x1, 2x1 or 2x2 over chroma 1x1 only")
    return hs, vs


def table_set_bytes(h):
    """The SQ_JPEG_TABLE_SET_BYTES block of a parsed stream's tables."""
    out = np.zeros(TABLE_SET_BYTES, dtype=np.uint8)
    quant = out[:512].view("<u2").reshape(4, 64)
    for tq, vals in h.quant.items():
        quant[tq] = vals
    for (tc, th), (counts, symbols) in h.huff.items():
        at = 512 + (tc * 2 + th) * 272
        out[at:at + 16] = np.frombuffer(counts, dtype=np.uint8)
        out[at + 16:at + 16 + len(symbols)] = np.frombuffer(symbols, dtype=np.uint8)
    return out.tobytes()


def selectors(h, what):
    """The selector word of a parsed stream: component c at bits 4c, quantisation table | DC table << 2 | AC table << 3."""
    sel = 0
    by_id = {cid: (td, ta) for cid, td, ta in h.scan}
    for c, (cid, _, _, tq) in enumerate(h.frame[4]):
        if cid not in by_id:
            raise WsiFormatError(f"{what}: SOS does not name component {cid} of the frame")
        td, ta = by_id[cid]
        if tq not in h.quant or (0, td) not in h.huff or (1, ta) not in h.huff or td > 1 or ta > 1:
            raise WsiFormatError(f"{what}: component {cid} names quantisation table {tq}, DC table {td}, AC table {ta}, not all defined")
        sel |= (tq | (td << 2) | (ta << 3)) << (4 * c)
    return sel


# ---- JPEG 2000 codestream headers ---------------------------------------------------------------------------------------
J2K_COMPRESSIONS = {33003: "Aperio JPEG 2000, YCbCr", 33005: "Aperio JPEG 2000, RGB"}
_J2K_MARKERS = {0x51: "SIZ", 0x52: "COD", 0x53: "COC", 0x5C: "QCD", 0x5D: "QCC", 0x5E: "RGN", 0x5F: "POC", 0x55: "TLM", 0x57: "PLM", 0x58: "PLT",
                0x60: "PPM", 0x61: "PPT", 0x63: "CRG", 0x64: "COM", 0x90: "SOT", 0x93: "SOD", 0x91: "SOP", 0x92: "EPH"}
_J2K_ORDERS = ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")
_J2K_STYLE_BITS = ("selective arithmetic coding bypass", "reset of context probabilities", "termination on each coding pass",
                   "vertically causal context", "predictable termination", "segmentation symbols")


class J2kHeader:
    """Main and tile-part header of one raw codestream: ``size`` (Xsiz, Ysiz), ``dx`` (chroma column sampling), the COD fields
    ``order``, ``layers``, ``mct``, ``levels``, ``xcb``, ``ycb``, ``reversible``, ``precincts`` [(PPx, PPy)] per resolution,
    ``quant`` per component (guard bits, style, [(exponent, mantissa)] per band, a derived style expanded), the byte range
    [body_start, body_end) of the packets, and ``params``, the SQ_J2K_PARAM_BYTES block of all that."""
    __slots__ = ("size", "dx", "order", "layers", "mct", "levels", "xcb", "ycb", "reversible", "precincts", "quant", "body_start",
                 "body_end", "params")


def _j2k_quant(what, name, style_byte, payload, levels):
    style, guard = style_byte & 31, style_byte >> 5
    bands = 3 * levels + 1
    if style == 0:
        if len(payload) < bands:
            raise WsiFormatError(f"{what}: {name} without quantisation lists {len(payload)} exponents, {bands} are needed for {levels} levels")
        steps = [(payload[i] >> 3, 0) for i in range(bands)]
    elif style in (1, 2):
        count = 1 if style == 1 else bands
        if len(payload) < 2 * count:
            raise WsiFormatError(f"{what}: {name} style {style} lists {len(payload) // 2} step sizes, {count} are needed")
        words = [(payload[2 * i] << 8) | payload[2 * i + 1] for i in range(count)]
        steps = [(v >> 11, v & 0x7FF) for v in words]
        if style == 1:                       # derived: exponent of band b is that of LL less the levels below it
            e0, m0 = steps[0]
            steps = [(e0, m0)] + [(e0 - r + 1, m0) for r in range(1, levels + 1) for _ in range(3)]
            if steps[-1][0] < 0:
                raise WsiFormatError(f"{what}: {name} derived exponent {e0} is too small for {levels} levels")
    else:
        raise WsiFormatError(f"{what}: {name} quantisation style {style}: 0 (none), 1 (derived) or 2 (expounded) only")
    for e, _ in steps:
        if not 0 <= guard + e - 1 <= _C["SQ_J2K_MAX_PLANES"]:
            raise WsiFormatError(f"{what}: {name} guard bits {guard} with exponent {e}: at most {_C['SQ_J2K_MAX_PLANES']} bit-planes")
    return guard, style, steps


def _j2k_coding(what, name, data, seg, end, has_precincts):
    """(levels, xcb, ycb, reversible, precincts) of the SPcod / SPcoc bytes at seg."""
    if end - seg < 5:
        raise WsiFormatError(f"{what}: {name} has {end - seg} coding-style bytes, 5 are needed")
    levels, xcb, ycb, style, wavelet = data[seg], data[seg + 1] + 2, data[seg + 2] + 2, data[seg + 3], data[seg + 4]
    if levels > 8:
        raise WsiFormatError(f"{what}: {name} with {levels} decomposition levels: 0..8 only")
    if data[seg + 1] > 4 or data[seg + 2] > 4:
        raise WsiFormatError(f"{what}: {name} code-block size {1 << xcb} x {1 << ycb}: 4..64 each only")
    if style:
        bits = ", ".join(_J2K_STYLE_BITS[i] if i < 6 else f"bit {i}" for i in range(8) if style >> i & 1)
        raise WsiFormatError(f"{what}: {name} code-block style {style:#x} ({bits}) is not supported: 0 only")
    if wavelet > 1:
        raise WsiFormatError(f"{what}: {name} wavelet {wavelet}: 0 (9/7) or 1 (5/3) only")
    precincts = [(15, 15)] * (levels + 1)
    if has_precincts:
        if end - seg < 5 + levels + 1:
            raise WsiFormatError(f"{what}: {name} lists {end - seg - 5} precinct sizes, {levels + 1} are needed")
        precincts = [(data[seg + 5 + r] & 15, data[seg + 5 + r] >> 4) for r in range(levels + 1)]
        for r, (px, py) in enumerate(precincts):
            if r and (px < 1 or py < 1):
                raise WsiFormatError(f"{what}: {name} precinct exponents ({px}, {py}) at resolution {r}: at least 1")
    return levels, xcb, ycb, wavelet, precincts


def parse_j2k(data, what="JPEG 2000 codestream"):
    """Walk the main header and the one tile-part header of a raw codestream (bytes): a ``J2kHeader``.  Whatever the decoder
    does not take is refused with a ``WsiFormatError`` naming the marker or field and its value (module docstring)."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0x4F:
        raise WsiFormatError(f"{what}: no SOC marker (ff 4f) at its start, it starts with {bytes(data[:4]).hex(' ')}")
    h = J2kHeader()
    h.size = None
    cod, qcd, coc, qcc, in_tile, psot, sot_at = None, None, {}, {}, False, 0, 0
    pos = 2
    while True:
        if pos + 2 > n:
            raise WsiFormatError(f"{what}: the header ends at byte {pos} before SOD")
        if data[pos] != 0xFF:
            raise WsiFormatError(f"{what}: byte {data[pos]:#x} at {pos} where a marker was expected")
        m = data[pos + 1]
        name = _J2K_MARKERS.get(m, f"marker {m:#x}")
        if m == 0x93:
            break
        if pos + 4 > n:
            raise WsiFormatError(f"{what}: {name} at {pos} runs past the end")
        length = (data[pos + 2] << 8) | data[pos + 3]
        seg, end = pos + 4, pos + 2 + length
        if length < 2 or end > n:
            raise WsiFormatError(f"{what}: {name} at {pos} of length {length} runs past the end")
        if m in (0x5E, 0x5F, 0x60, 0x61, 0x55, 0x57):
            raise WsiFormatError(f"{what}: {name} marker segment ({m:#x}) is not supported")
        if m == 0x51:
            if end - seg < 36:
                raise WsiFormatError(f"{what}: SIZ of {end - seg} bytes, at least 36 are needed")
            xs, ys, xo, yo, xt, yt, xto, yto, nc = struct.unpack_from(">8IH", data, seg + 2)
            if nc != 3:
                raise WsiFormatError(f"{what}: SIZ Csiz = {nc} components: 3 only")
            if end - seg < 36 + 9:
                raise WsiFormatError(f"{what}: SIZ of 3 components has {end - seg} bytes, 45 are needed")
            comps = [(data[seg + 36 + 3 * i], data[seg + 37 + 3 * i], data[seg + 38 + 3 * i]) for i in range(3)]
            if any(c[0] != 7 for c in comps):
                raise WsiFormatError(f"{what}: SIZ Ssiz = {[c[0] for c in comps]}: 8 bits unsigned (7) only")
            if (xo, yo, xto, yto) != (0, 0, 0, 0):
                raise WsiFormatError(f"{what}: SIZ image and tile offsets {(xo, yo, xto, yto)}: 0 only")
            if xt < xs or yt < ys:
                raise WsiFormatError(f"{what}: SIZ tiles of {xt} x {yt} in an image of {xs} x {ys}: more than one tile is not supported")
            sampling = [(c[1], c[2]) for c in comps]
            if sampling not in ([(1, 1)] * 3, [(1, 1), (2, 1), (2, 1)]):
                raise WsiFormatError(f"{what}: SIZ component sampling (XRsiz, YRsiz) = {sampling}: 1x1 for all, or 1x1, 2x1, 2x1 only")
            h.size, h.dx = (xs, ys), sampling[1][0]
        elif m == 0x52:
            if end - seg < 5:
                raise WsiFormatError(f"{what}: COD of {end - seg} bytes")
            scod, order, layers, mct = data[seg], data[seg + 1], (data[seg + 2] << 8) | data[seg + 3], data[seg + 4]
            if scod & 2:
                raise WsiFormatError(f"{what}: COD Scod = {scod:#x}: SOP marker segments are not supported")
            if scod & 4:
                raise WsiFormatError(f"{what}: COD Scod = {scod:#x}: EPH markers are not supported")
            if order > 4:
                raise WsiFormatError(f"{what}: COD progression order {order}: 0..4 only")
            if not 1 <= layers <= 32:
                raise WsiFormatError(f"{what}: COD with {layers} quality layers: 1..32 only")
            if mct > 1:
                raise WsiFormatError(f"{what}: COD multiple component transform {mct}: 0 or 1 only")
            cod = (order, layers, mct) + _j2k_coding(what, "COD", data, seg + 5, end, scod & 1)
        elif m == 0x53:
            if end - seg < 2 or data[seg] > 2:
                raise WsiFormatError(f"{what}: COC for component {data[seg] if end > seg else '?'}")
            coc[data[seg]] = _j2k_coding(what, "COC", data, seg + 2, end, data[seg + 1] & 1)
        elif m == 0x5C:
            qcd = (data[seg], bytes(data[seg + 1:end]))
        elif m == 0x5D:
            if end - seg < 2 or data[seg] > 2:
                raise WsiFormatError(f"{what}: QCC for component {data[seg] if end > seg else '?'}")
            qcc[data[seg]] = (data[seg + 1], bytes(data[seg + 2:end]))
        elif m == 0x90:
            if in_tile:
                raise WsiFormatError(f"{what}: a second SOT: one tile-part only")
            if end - seg < 8:
                raise WsiFormatError(f"{what}: SOT of {end - seg} bytes, 8 are needed")
            isot, psot, tp, tn = struct.unpack_from(">HIBB", data, seg)
            if isot != 0 or tp != 0 or tn > 1:
                raise WsiFormatError(f"{what}: SOT tile {isot}, tile-part {tp} of {tn}: one tile in one tile-part only")
            in_tile, sot_at = True, pos
        elif m in (0x91, 0x92):
            raise WsiFormatError(f"{what}: {name} in a header")
        # COM, PLT, CRG and unknown segments are skipped
        pos = end
    if h.size is None or cod is None or qcd is None or not in_tile:
        missing = [k for k, v in (("SIZ", h.size), ("COD", cod), ("QCD", qcd), ("SOT", in_tile or None)) if v is None]
        raise WsiFormatError(f"{what}: SOD without {', '.join(missing)} before it")
    h.order, h.layers, h.mct, h.levels, h.xcb, h.ycb, wavelet, h.precincts = cod
    h.reversible = wavelet
    for c, other in coc.items():
        if other != cod[3:]:
            raise WsiFormatError(f"{what}: COC for component {c} differs from COD ({other} against {cod[3:]}): one coding style for all components only")
    if h.mct and h.dx != 1:
        raise WsiFormatError(f"{what}: COD multiple component transform with SIZ sampling 2x1: the transform needs 1x1 everywhere")
    h.quant = []
    for c in range(3):
        style_byte, payload = qcc.get(c, qcd)
        guard, style, steps = _j2k_quant(what, "QCC" if c in qcc else "QCD", style_byte, payload, h.levels)
        if bool(h.reversible) != (style == 0):
            raise WsiFormatError(f"{what}: quantisation style {style} with wavelet {wavelet}: 5/3 goes without quantisation, 9/7 with")
        h.quant.append((guard, style, steps))
    h.body_start = pos + 2
    h.body_end = min(n, sot_at + psot) if psot else n
    if h.body_end - 2 >= h.body_start and data[h.body_end - 2] == 0xFF and data[h.body_end - 1] == 0xD9 and not psot:
        h.body_end -= 2
    if psot and sot_at + psot + 2 <= n and (data[sot_at + psot], data[sot_at + psot + 1]) == (0xFF, 0x90):
        raise WsiFormatError(f"{what}: a second SOT behind the first tile-part: one tile-part only")
    if h.body_end <= h.body_start:
        raise WsiFormatError(f"{what}: no packet bytes behind SOD")
    for r, (px, py) in enumerate(h.precincts):
        cw = -(-h.size[0] // h.dx)
        rw, rh = -(-cw // (1 << (h.levels - r))), -(-h.size[1] // (1 << (h.levels - r)))
        rw0 = -(-h.size[0] // (1 << (h.levels - r)))
        count = max(-(-rw0 // (1 << px)), -(-rw // (1 << px))) * -(-rh // (1 << py))
        if h.order >= 2 and count != 1:
            raise WsiFormatError(f"{what}: COD progression {_J2K_ORDERS[h.order]} with {count} precincts at resolution {r}: positional "
                                 f"progressions with a single precinct per resolution only")
        if count > _C["SQ_J2K_MAX_PRECINCTS"]:
            raise WsiFormatError(f"{what}: COD precinct exponents ({px}, {py}) make {count} precincts at resolution {r}: at most {_C['SQ_J2K_MAX_PRECINCTS']}")
    words = np.zeros(_C["SQ_J2K_PARAM_BYTES"] // 4, dtype="<i4")
    words[:9] = (_C["SQ_J2K_PARAM_MAGIC"], h.dx, h.levels, h.reversible, h.mct, h.layers, h.order, h.xcb, h.ycb)
    words[9:18] = 15 | (15 << 4)
    for r, (px, py) in enumerate(h.precincts):
        words[9 + r] = px | (py << 4)
    for c, (guard, style, steps) in enumerate(h.quant):
        at = 18 + 52 * c
        words[at], words[at + 1] = guard, style
        words[at + 2:at + 2 + 2 * len(steps)] = np.asarray(steps, dtype="<i4").reshape(-1)
    h.params = words.tobytes()
    return h


class _Level:
    __slots__ = ("width", "height", "tile_w", "tile_h", "tiles_x", "tiles_y", "offsets", "counts", "base", "transform", "hs", "vs",
                 "index", "info", "shared", "codec", "compression", "caps", "predictor")


class TiffSlide:
    """``openslide.OpenSlide(path)`` for a JPEG-tiled TIFF / SVS file (module docstring).  ``read_region`` returns an RGBA
    ``PIL.Image``; ``read_regions`` the same pixels for a batch as a device tensor.  Opening and the properties need no GPU.
    ``entropy``: how the scans of JPEG tiles are decoded -- 'serial' (one lane per tile, ``sq_jpeg_decode_tiles``) or 'split'
    (the 64 lanes of a wave on one tile's scan, ``sq_jpeg_decode_tiles_split``: the same bytes whatever the file holds; tiles
    with restart intervals still decode on one lane).  ``sub_bytes``, an expert knob of 'split': the bytes of scan per lane and
    round, a multiple of 4 in SQ_JPEG_SPLIT_SUB_MIN..SQ_JPEG_SPLIT_SUB_MAX, or 0 for the library's default.  JPEG 2000, LZW and
    uncompressed levels ignore both."""

    def __init__(self, path, device="cuda:0", workspace_budget=DEFAULT_WORKSPACE_BUDGET, entropy="serial", *, sub_bytes=0):
        if entropy not in ("serial", "split"):
            raise ValueError(f"entropy={entropy!r}: 'serial' or 'split'")
        sub_bytes = int(sub_bytes)
        if sub_bytes and not (_C["SQ_JPEG_SPLIT_SUB_MIN"] <= sub_bytes <= _C["SQ_JPEG_SPLIT_SUB_MAX"] and sub_bytes % 4 == 0):
            raise ValueError(f"sub_bytes={sub_bytes}: a multiple of 4 in {_C['SQ_JPEG_SPLIT_SUB_MIN']}..{_C['SQ_JPEG_SPLIT_SUB_MAX']}, or 0 "
                             f"for the library's default")
        self.path, self.device, self.workspace_budget = path, device, int(workspace_budget)
        self.entropy, self.sub_bytes = entropy, sub_bytes
        self.lzw_mode = LZW_MODE                # how LZW tiles are decoded; the measurement tool and the tests switch it, no CLI does
        self._fd = os.open(path, os.O_RDONLY)
        self._pinned = None
        self.last_batch_tiles = []           # (tile_x, tile_y) of every tile decode of the last read_regions call, chunk by chunk
        try:
            self._size = os.fstat(self._fd).st_size
            ifds, self.bigtiff = read_ifds(self._fd, self._size)
            self._levels = [self._level(i, t) for i, t in enumerate(ifds) if 322 in t or 323 in t]
            if not self._levels:
                raise WsiFormatError("no tiled IFD (TileWidth / TileLength) in the file: stripped images are not levels")
            self._levels.sort(key=lambda lv: -lv.width)
            self.level_count = len(self._levels)
            self.level_dimensions = tuple((lv.width, lv.height) for lv in self._levels)
            self.dimensions = self.level_dimensions[0]
            self.level_downsamples = tuple(self.dimensions[0] / lv.width for lv in self._levels)
            self.properties = self._properties(ifds[self._levels[0].index].get(270, b""))
            self.properties["openslide.level-count"] = str(self.level_count)         # a string, as OpenSlide gives it
        except Exception:
            os.close(self._fd)
            self._fd = None
            raise

    # -- container --
    def _level(self, index, tags):
        what = f"IFD {index}"

        def need(tag, allowed, text):
            v = tags.get(tag)
            v = tuple(int(x) for x in v) if v is not None else None
            if v is None or any(x not in allowed for x in v):
                raise WsiFormatError(f"{what}: {_TAG_NAMES[tag]} = {v if v is None or len(v) != 1 else v[0]}: {text}")
            return v
        comp = _one(tags, 259, 1)
        lossless = comp in LZW_COMPRESSIONS
        if comp != 7 and comp not in J2K_COMPRESSIONS and not lossless:
            name = {8: " (deflate)", 32946: " (deflate)", 34712: " (JPEG 2000)"}.get(comp, "")
            raise WsiFormatError(f"{what}: Compression = {comp}{name} is not supported: 7 (JPEG), 33003 or 33005 (Aperio JPEG 2000), 5 (LZW) or "
                                 f"1 (uncompressed) only")
        if lossless:                        # chunky RGB as stored: no colour transform, no subsampling, no alpha
            what_comp = f"{what}: Compression = {comp} ({LZW_COMPRESSIONS[comp]})"
            if _one(tags, 262) != 2:
                raise WsiFormatError(f"{what_comp} with PhotometricInterpretation = {_one(tags, 262)}: 2 (RGB) only")
            if 338 in tags:
                raise WsiFormatError(f"{what_comp} with ExtraSamples = {tuple(int(x) for x in tags[338])}: three samples without alpha only")
            if _one(tags, 266, 1) != 1:
                raise WsiFormatError(f"{what_comp} with FillOrder = {_one(tags, 266)}: 1 (most significant bit first) only")
            if _one(tags, 317, 1) not in (1, 2):
                kind = " (floating point)" if _one(tags, 317) == 3 else ""
                raise WsiFormatError(f"{what_comp} with Predictor = {_one(tags, 317)}{kind}: 1 (none) or 2 (horizontal differencing) only")
        need(258, (8,), "8 bits per sample only")
        if len(need(277, (3,), "3 samples per pixel only")) != 1 or len(tags[258]) != 3:
            raise WsiFormatError(f"{what}: BitsPerSample = {tuple(int(x) for x in tags[258])}: three samples of 8 bits only")
        if _one(tags, 284, 1) != 1:
            raise WsiFormatError(f"{what}: PlanarConfiguration = {_one(tags, 284)}: 1 (chunky) only")
        photometric = need(262, (2, 6), "2 (RGB) or 6 (YCbCr) only")[0] if comp == 7 else None      # not consulted for JPEG 2000
        lv = _Level()
        lv.codec, lv.compression, lv.caps = ("jpeg" if comp == 7 else "lzw" if comp == 5 else "raw" if comp == 1 else "j2k"), comp, None
        lv.predictor = _one(tags, 317, 1) if lossless else 1
        lv.index, lv.width, lv.height = index, _one(tags, 256, 0), _one(tags, 257, 0)
        lv.tile_w, lv.tile_h = _one(tags, 322, 0), _one(tags, 323, 0)
        if lv.width < 1 or lv.height < 1:
            raise WsiFormatError(f"{what}: ImageWidth = {lv.width}, ImageLength = {lv.height}")
        for tag, v in ((322, lv.tile_w), (323, lv.tile_h)):
            if v % 16 or not 16 <= v <= MAX_TILE:
                raise WsiFormatError(f"{what}: {_TAG_NAMES[tag]} = {v}: a multiple of 16 in 16..{MAX_TILE} only")
        lv.tiles_x, lv.tiles_y = -(-lv.width // lv.tile_w), -(-lv.height // lv.tile_h)
        if 324 not in tags or 325 not in tags or len(tags[324]) != lv.tiles_x * lv.tiles_y or len(tags[325]) != len(tags[324]):
            raise WsiFormatError(f"{what}: TileOffsets / TileByteCounts must have {lv.tiles_x * lv.tiles_y} entries each")
        lv.offsets, lv.counts = tags[324].astype(np.int64), tags[325].astype(np.int64)
        if (lv.counts == 0).any():
            t = int(np.flatnonzero(lv.counts == 0)[0])
            raise WsiFormatError(f"{what}: TileByteCounts[{t}] = 0 (tile {t % lv.tiles_x}, {t // lv.tiles_x}): empty tiles are not supported")
        lv.transform = 1 if (photometric == 6 or comp == 33003) else 0
        lv.base = parse_jpeg(bytes(tags[347]), what=f"{what} JPEGTables") if (347 in tags and comp == 7) else None
        lv.shared = table_set_bytes(lv.base) if lv.base is not None else None      # ONE object for every tile without tables of its own
        lv.info = {}
        lv.hs, lv.vs = (1, 1) if lossless else (None, None)         # the planes are written at full resolution
        if comp == 1 and (lv.counts != lv.tile_w * lv.tile_h * 3).any():
            t = int(np.flatnonzero(lv.counts != lv.tile_w * lv.tile_h * 3)[0])
            raise WsiFormatError(f"{what}: Compression = 1 (uncompressed) with TileByteCounts[{t}] = {int(lv.counts[t])} (tile {t % lv.tiles_x}, "
                                 f"{t // lv.tiles_x}): tiles of {lv.tile_w} x {lv.tile_h} x 3 samples hold {lv.tile_w * lv.tile_h * 3} bytes")
        past = np.flatnonzero(lv.offsets + lv.counts > self._size)
        if past.size == 0:                  # a range past the end of the file is reported when that tile is read
            self._tile_info(lv, 0, level_name=what)
        return lv

    def _tile_info(self, lv, t, level_name=None):
        """(file offset of the scan, its length, table-set bytes, restart interval, selectors) of tile t, parsed once.  A tile
        without DQT / DHT of its own gets the level's shared table-set object (``lv.shared``, from JPEGTables), not a copy."""
        got = lv.info.get(t)
        if got is not None:
            return got
        what = f"{level_name or f'IFD {lv.index}'} tile ({t % lv.tiles_x}, {t // lv.tiles_x})"
        off, count = int(lv.offsets[t]), int(lv.counts[t])
        if off < 0 or off + count > self._size:
            raise WsiFormatError(f"{what}: TileOffsets = {off} with TileByteCounts = {count} runs past the end of the file ({self._size} bytes)")
        if lv.codec in ("lzw", "raw"):       # the whole tile is the scan; an LZW stream must open with the Clear code (256 in 9 bits)
            first = os.pread(self._fd, 2, off)
            if lv.codec == "lzw" and (len(first) < 2 or first[0] != 0x80 or first[1] & 0x80):
                raise WsiFormatError(f"IFD {lv.index}: Compression = 5 (LZW) but {what} starts with bytes {first.hex(' ')}, not with the Clear code "
                                     f"(80 00 in nine bits): old-style LZW (least significant bit first, no Clear at the start) is not supported")
            got = lv.info[t] = (off, count, b"", 0, 0)
            return got
        data = os.pread(self._fd, count, off)
        if lv.codec == "j2k":
            return self._j2k_tile_info(lv, t, what, off, data)
        h = parse_jpeg(data, lv.base, what)
        if h.frame is None or h.scan is None:
            raise WsiFormatError(f"{what}: no SOF0 / SOS in the tile's stream")
        if (h.frame[3], h.frame[2]) != (lv.tile_w, lv.tile_h):
            raise WsiFormatError(f"{what}: SOF0 frame of {h.frame[3]} x {h.frame[2]} pixels in tiles of {lv.tile_w} x {lv.tile_h}: they must be equal")
        hs, vs = _sampling(h.frame, what)
        if lv.hs is None:
            lv.hs, lv.vs = hs, vs
        elif (hs, vs) != (lv.hs, lv.vs):
            raise WsiFormatError(f"{what}: SOF0 luma sampling {hs}x{vs} where the level's first tile has {lv.hs}x{lv.vs}")
        sel = selectors(h, what)
        tables = lv.shared if (lv.shared is not None and not h.own_tables) else table_set_bytes(h)
        got = (off + h.scan_start, h.scan_end - h.scan_start, tables, h.restart, sel)
        if got[1] < 1:
            raise WsiFormatError(f"{what}: an empty entropy-coded segment")
        lv.info[t] = got
        return got

    def _j2k_tile_info(self, lv, t, what, off, data):
        """``_tile_info`` of a JPEG 2000 tile: (file offset of the packets, their length, parameter-set bytes, 0, 0)."""
        if data[:2] != b"\xff\x4f":
            found = "a JPEG stream (SOI)" if data[:2] == b"\xff\xd8" else ("a JP2 file (boxes)" if data[4:8] == b"jP  " else f"bytes {data[:4].hex(' ')}")
            raise WsiFormatError(f"IFD {lv.index}: Compression = {lv.compression} ({J2K_COMPRESSIONS[lv.compression]}) but {what} holds {found} "
                                 f"where a raw codestream (SOC, ff 4f) was expected")
        h = parse_j2k(data, what)
        if h.size != (lv.tile_w, lv.tile_h):
            raise WsiFormatError(f"{what}: SIZ image of {h.size[0]} x {h.size[1]} pixels in tiles of {lv.tile_w} x {lv.tile_h}: they must be equal")
        lv.hs, lv.vs = 1, 1                  # the planes are written at full resolution
        got = (off + h.body_start, h.body_end - h.body_start, h.params, 0, 0)
        lv.info[t] = got
        return got

    @staticmethod
    def _properties(description):
        text = bytes(description).split(b"\0")[0].decode("latin-1")
        props = {"openslide.vendor": "aperio" if text.startswith("Aperio") else "generic-tiff"}
        if text:
            props["tiff.ImageDescription"] = text
        for part in text.split("|")[1:]:
            key, eq, value = part.partition("=")
            if eq:
                props[f"aperio.{key.strip()}"] = value.strip()
        if "aperio.MPP" in props:
            props["openslide.mpp-x"] = props["openslide.mpp-y"] = props["aperio.MPP"]
        return props

    def tile_ranges(self, level):
        """(offsets, byte counts) of the level's tiles as the file lists them, row-major."""
        lv = self._levels[level]
        return lv.offsets.copy(), lv.counts.copy()

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None
        self._pinned = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- pixels --
    def _origin(self, level, location):
        ds = self.dimensions[0] / self._levels[level].width
        return int(location[0] / ds), int(location[1] / ds)

    def read_regions(self, locations, level, size):
        """uint8 [k, h, w, 4] on ``self.device``: region i is ``read_region(locations[i], level, size)``.  The tiles the batch
        touches are decoded once per chunk; a batch is cut between regions into chunks whose device workspace (planes,
        coefficients, uploaded bytes) stays under ``workspace_budget`` bytes, and a batch that fits decodes every tile once.
        Outside the budget: the returned tensor itself (k h w 4 bytes), and a single region whose own tiles need more than the
        budget -- a region is never split, so it is decoded in one chunk whatever it takes (the whole-level read of the slide
        mask is one).  A chunk's scans are addressed by int32 offsets: chunks are cut below 2 GiB of scan bytes, and one region
        above that is refused with a ValueError.  The tile bytes go up in one pinned buffer with the tile table.  A tile that does not decode raises ``TileDecodeError`` (a RuntimeError naming
        the level and the tile) after the whole batch has run; every other tile of the batch is unaffected."""
        import torch
        _lib.require_gpu()
        if self._fd is None:
            raise ValueError("the slide is closed")
        if not 0 <= int(level) < self.level_count:
            raise ValueError(f"level {level}: the slide has levels 0..{self.level_count - 1}")
        lv = self._levels[int(level)]
        w, h = int(size[0]), int(size[1])
        if w < 1 or h < 1 or w > _C["SQ_JPEG_MAX_REGION"] or h > _C["SQ_JPEG_MAX_REGION"]:
            raise ValueError(f"region size {size}: extents in 1..{_C['SQ_JPEG_MAX_REGION']}")
        origins = [self._origin(level, xy) for xy in locations]
        if any(abs(x) >= 1 << 30 or abs(y) >= 1 << 30 for x, y in origins):
            raise ValueError("region origin beyond 2^30 pixels")
        k = len(origins)
        dev = torch.device(self.device)
        out = torch.empty((k, h, w, 4), dtype=torch.uint8, device=dev)
        self.last_batch_tiles = []
        if k == 0:
            return out
        touched = []
        for x0, y0 in origins:
            tx0, tx1 = max(x0, 0) // lv.tile_w, min(x0 + w - 1, lv.width - 1) // lv.tile_w
            ty0, ty1 = max(y0, 0) // lv.tile_h, min(y0 + h - 1, lv.height - 1) // lv.tile_h
            touched.append([ty * lv.tiles_x + tx for ty in range(ty0, ty1 + 1) for tx in range(tx0, tx1 + 1)]
                           if x0 < lv.width and y0 < lv.height and x0 + w > 0 and y0 + h > 0 else [])
        L = _lib.lib()
        first = self._tile_info(lv, 0)                                      # fixes the level's sampling
        if lv.codec in ("lzw", "raw"):
            per_tile = L.sq_lzw_workspace_bytes(2, lv.tile_w, lv.tile_h, lv.compression) - L.sq_lzw_workspace_bytes(1, lv.tile_w, lv.tile_h, lv.compression) \
                + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, 1, 1) + int(lv.counts.max())
        elif lv.codec == "j2k":             # the records of the first tile's parameter set stand for the level's in this estimate
            caps = self._j2k_caps(lv, [first[2]])
            per_tile = L.sq_j2k_workspace_bytes(2, lv.tile_w, lv.tile_h, *caps, 16) - L.sq_j2k_workspace_bytes(1, lv.tile_w, lv.tile_h, *caps, 16) \
                + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, 1, 1) + 2 * int(lv.counts.max())
        else:
            per_tile = L.sq_jpeg_workspace_bytes(2, 1, lv.tile_w, lv.tile_h, lv.hs, lv.vs) - L.sq_jpeg_workspace_bytes(1, 1, lv.tile_w, lv.tile_h, lv.hs, lv.vs) \
                + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, lv.hs, lv.vs) + int(lv.counts.max())
        max_tiles = max(1, min(self.workspace_budget // per_tile, SCAN_BYTES_MAX // (int(lv.counts.max()) + 3)))
        failures, start = [], 0
        while start < k:
            tiles, stop = set(), start
            while stop < k:
                new = [t for t in touched[stop] if t not in tiles]
                if stop > start and len(tiles) + len(new) > max_tiles:
                    break
                tiles.update(new)
                stop += 1
            failures += self._decode_chunk(lv, level, sorted(tiles), origins[start:stop], out[start:stop])
            start = stop
        if failures:
            table = J2K_STATUS_NAMES if lv.codec == "j2k" else LZW_STATUS_NAMES if lv.codec in ("lzw", "raw") else STATUS_NAMES
            names = ", ".join(f"({tx}, {ty}): {table.get(st, st)}" for _, tx, ty, st in failures[:8])
            bad = {ty * lv.tiles_x + tx for _, tx, ty, _ in failures}
            first = min(i for i, t in enumerate(touched) if bad & set(t))
            raise TileDecodeError(f"{self.path}: level {level}: {len(failures)} tile(s) did not decode: tile {names}", failures, out, first)
        return out

    def _plan(self, lv, tiles):
        """The device inputs of a set of tiles (row-major tile numbers) but for the scan bytes: the slot order (longest scan
        first, so that the lanes of a wave end together), the tile table, the distinct table sets, the size of the scans buffer
        and the level's tile -> slot map."""
        infos = [self._tile_info(lv, t) for t in tiles]
        order = sorted(range(len(tiles)), key=lambda i: -infos[i][1])
        set_index, sets = {}, []
        words = {"j2k": J2K_TILE_WORDS, "lzw": LZW_TILE_WORDS, "raw": LZW_TILE_WORDS}.get(lv.codec, TILE_WORDS)
        table = np.zeros((len(tiles), words), dtype=np.int32)
        slot_map = np.full(lv.tiles_x * lv.tiles_y, -1, dtype=np.int32)
        at = 0
        for slot, i in enumerate(order):
            off, length, tables, restart, sel = infos[i]
            if tables not in set_index:
                set_index[tables] = len(sets)
                sets.append(tables)
            if at + length > SCAN_BYTES_MAX:
                raise ValueError(f"{self.path}: the tiles of one region hold more than {SCAN_BYTES_MAX} bytes of scans (the tile table's "
                                 f"offsets are int32): read the region in parts")
            table[slot] = (at, length, set_index[tables], restart, sel, 0, 0, 0)[:words]
            slot_map[tiles[i]] = slot
            at += (length + 3) & ~3
        return order, table, sets, max((at + 15) & ~15, 16), slot_map

    def _read_scans(self, lv, level, tiles, order, table, host):
        """The entropy-coded bytes of the planned tiles from the file into `host` (uint8 numpy [scans_bytes])."""
        view = memoryview(host)
        for slot, i in enumerate(order):
            a, length = int(table[slot, 0]), int(table[slot, 1])
            got = os.preadv(self._fd, [view[a:a + length]], self._tile_info(lv, tiles[i])[0])
            if got != length:
                raise WsiFormatError(f"{self.path}: level {level} tile ({tiles[i] % lv.tiles_x}, {tiles[i] // lv.tiles_x}): read {got} of {length} bytes")
            host[a + length:a + ((length + 3) & ~3)] = 0

    def _j2k_caps(self, lv, sets):
        """(code-blocks, tag-tree nodes, precinct-bands) a tile of `sets` (parameter-set byte strings) needs at most: the
        library's own count (sq_j2k_layout, host only), kept per set."""
        import ctypes
        if lv.caps is None:
            lv.caps = {}
        for params in sets:
            if params not in lv.caps:
                counts = (ctypes.c_int32 * 3)()
                _lib.check(_lib.lib().sq_j2k_layout(params, lv.tile_w, lv.tile_h, ctypes.cast(counts, ctypes.c_void_p)))
                lv.caps[params] = tuple(counts)
        return tuple(max(1, max(lv.caps[p][i] for p in sets)) for i in range(3))

    def tile_job(self, level, tiles=None):
        """What ``read_regions`` uploads for `tiles` (row-major tile numbers, default all) of `level`, on the host: a dict with
        ``codec`` ('jpeg' or 'j2k'), ``geom`` (tile_w, tile_h, hs, vs), ``transform``, ``tiles`` (the tile number of every slot),
        ``table`` int32 [n, 8] (JPEG 2000: [n, 4]), ``sets`` (list of table-set or parameter-set byte strings) and ``scans``
        (uint8 array: the scans, or the packet bytes); JPEG 2000 adds ``caps``, the record counts the workspace is sized by.
        LZW and uncompressed levels ('lzw', 'raw') have no sets: ``codec``, ``geom``, ``predictor``, ``tiles``, ``table`` int32
        [n, 4] and ``scans`` (the tiles' bytes as the file holds them).  Needs no GPU: the host check programs and the tests read it."""
        lv = self._levels[level]
        tiles = list(range(lv.tiles_x * lv.tiles_y)) if tiles is None else list(tiles)
        order, table, sets, scans_bytes, _ = self._plan(lv, tiles)
        scans = np.zeros(scans_bytes, dtype=np.uint8)
        self._read_scans(lv, level, tiles, order, table, scans)
        if lv.codec in ("lzw", "raw"):       # no table sets: the predictor is all a tile needs besides its bytes
            return dict(codec=lv.codec, geom=(lv.tile_w, lv.tile_h, 1, 1), predictor=lv.predictor, tiles=[tiles[i] for i in order], table=table,
                        scans=scans)
        job = dict(codec=lv.codec, geom=(lv.tile_w, lv.tile_h, lv.hs, lv.vs), transform=lv.transform, tiles=[tiles[i] for i in order], table=table,
                   sets=sets, scans=scans)
        if lv.codec == "j2k":
            job["caps"] = self._j2k_caps(lv, sets)
        return job

    def _decode_chunk(self, lv, level, tiles, origins, out):
        """Decode `tiles` (row-major tile numbers) and compose `origins` into `out`; returns the failing tiles."""
        import torch
        L = _lib.lib()
        dev = out.device
        k, h, w = out.shape[0], out.shape[1], out.shape[2]
        regions = np.asarray(origins, dtype=np.int32).reshape(-1, 2)
        if not tiles:
            out.zero_()
            return []
        order, table, sets, scans_bytes, slot_map = self._plan(lv, tiles)
        n = len(tiles)
        parts = [table.tobytes(), b"".join(sets), slot_map.tobytes(), regions.tobytes()]
        parts = [p + b"\0" * (-len(p) % 16) for p in parts]                   # the scans behind them start 16-byte aligned
        head = sum(len(p) for p in parts)
        total = head + scans_bytes
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
        host = self._pinned.numpy()
        host[:head] = np.frombuffer(b"".join(parts), dtype=np.uint8)
        self._read_scans(lv, level, tiles, order, table, host[head:total])
        self.last_batch_tiles += [(t % lv.tiles_x, t // lv.tiles_x) for t in tiles]
        blob = self._pinned[:total].to(dev, non_blocking=True)
        o_sets = len(parts[0])
        o_slots = o_sets + len(parts[1])
        o_regions = o_slots + len(parts[2])
        geom = (lv.tile_w, lv.tile_h, lv.hs, lv.vs)
        planes = torch.empty(_lib.need(L.sq_jpeg_planes_bytes, n, *geom), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        if lv.codec in ("lzw", "raw"):
            need = _lib.need(L.sq_lzw_workspace_bytes, n, lv.tile_w, lv.tile_h, lv.compression)
            _lib.call("sq_lzw_decode_tiles", dev, blob[head:], scans_bytes, blob, n, lv.tile_w, lv.tile_h, lv.compression, lv.predictor, self.lzw_mode,
                      planes, status, workspace=need)
        elif lv.codec == "j2k":
            caps = self._j2k_caps(lv, sets)
            need = _lib.need(L.sq_j2k_workspace_bytes, n, lv.tile_w, lv.tile_h, *caps, scans_bytes)
            _lib.call("sq_j2k_decode_tiles", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), lv.tile_w, lv.tile_h, *caps,
                      planes, status, workspace=need)
        elif self.entropy == "split":
            need = _lib.need(L.sq_jpeg_split_workspace_bytes, n, len(sets), *geom)
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)      # in the argument list: sub_bytes stands behind the workspace pair
            _lib.call("sq_jpeg_decode_tiles_split", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), *geom, planes, status,
                      scratch, need, self.sub_bytes)
        else:
            need = _lib.need(L.sq_jpeg_workspace_bytes, n, len(sets), *geom)
            _lib.call("sq_jpeg_decode_tiles", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), *geom, planes, status, workspace=need)
        _lib.call("sq_jpeg_compose_regions", dev, planes, n, *geom, lv.transform, blob[o_slots:], lv.tiles_x, lv.tiles_y, lv.width, lv.height,
                  blob[o_regions:], k, h, w, out)
        st = status.cpu().numpy()            # waits for the chunk: the pinned buffer may be written again
        return [(level, tiles[order[s]] % lv.tiles_x, tiles[order[s]] // lv.tiles_x, int(st[s])) for s in np.flatnonzero(st)]

    def read_region(self, location, level, size):
        """``openslide.OpenSlide.read_region``: an RGBA ``PIL.Image`` of `size` = (width, height) pixels of `level` whose corner
        is at `location` in level-0 pixels (module docstring: a fractional level origin is truncated, not interpolated).
        ``read_regions`` of one region, downloaded."""
        from PIL import Image
        return Image.fromarray(self.read_regions([location], level, size)[0].cpu().numpy(), "RGBA")


MISSING_OPENSLIDE = ("openslide-python is required to read whole-slide images (pip install openslide-python); "
                     "sequoia-pub_amd.patchgen.extract_patches and embed_slide also accept any object with OpenSlide's interface.  "
                     "JPEG-, JPEG 2000-, LZW-tiled and uncompressed tiled TIFF and Aperio SVS files open without it: pass --reader tiff.")


def open_slide(path, reader="openslide", device="cuda:0", entropy="serial"):
    """The slide object of the CLIs' ``--reader`` flag: 'tiff' is ``TiffSlide``, 'openslide' is ``openslide.OpenSlide`` (and a
    SystemExit that points to ``--reader tiff`` when openslide-python is not installed).  ``entropy`` ('serial' or 'split', the
    CLIs' ``--jpeg_entropy``) is ``TiffSlide``'s; the openslide reader has no use for it."""
    if entropy not in ("serial", "split"):
        raise ValueError(f"entropy={entropy!r}: 'serial' or 'split'")
    if reader == "tiff":
        return TiffSlide(path, device=device, entropy=entropy)
    if reader != "openslide":
        raise ValueError(f"reader={reader!r}: 'openslide' or 'tiff'")
    try:
        import openslide
    except ImportError:
        raise SystemExit(MISSING_OPENSLIDE) from None
    return openslide.OpenSlide(path)


