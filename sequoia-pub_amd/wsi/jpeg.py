"""JPEG tiles (compression 7): the marker parser and the codec of a JPEG-tiled TIFF / Aperio SVS level.  The tiles are decoded
by the library on the device (``sq_jpeg_decode_tiles``, ``sq_jpeg_compose_regions``: csrc/jpegdec.hip), every byte libjpeg's.

A tiled IFD of compression 7 must have, besides what the container asks of every level (package docstring), photometric 2
(RGB) or 6 (YCbCr), and baseline frames of exactly the tile extent with luma sampling 1x1, 2x1 or 2x2 over chroma 1x1.
Everything else -- progressive, arithmetic or 12-bit frames, 1 or 4 components, other samplings -- is refused with a
``WsiFormatError`` that names the tag or marker and its value.  The TIFF photometric tag decides the colour transform as libtiff
does (6: YCbCr -> RGB, 2: components as stored); JFIF and Adobe markers of the stream are ignored.

How the scans are decoded is the slide's ``entropy``: 'serial' (one lane per tile, ``sq_jpeg_decode_tiles``) or 'split' (the 64
lanes of a wave on one tile's scan, ``sq_jpeg_decode_tiles_split``), with the slide's ``sub_bytes``; both are read when a chunk
is decoded."""
import os

import numpy as np

from . import WsiFormatError
from .. import _lib
from .._abi import CONSTANTS as _C
from .tiff import Codec, TileInfo, check_samples, need_tag

TILE_WORDS, TABLE_SET_BYTES = _C["SQ_JPEG_TILE_WORDS"], _C["SQ_JPEG_TABLE_SET_BYTES"]
STATUS_NAMES = {_C["SQ_JPEG_BAD_TABLE"]: "a Huffman table that is no prefix code or a missing table set",
                _C["SQ_JPEG_BAD_RANGE"]: "a scan range outside the uploaded bytes",
                _C["SQ_JPEG_TRUNCATED"]: "the scan ends before its last MCU",
                _C["SQ_JPEG_BAD_CODE"]: "a code that matches no Huffman table entry",
                _C["SQ_JPEG_BAD_COEF"]: "a zero run past coefficient 63",
                _C["SQ_JPEG_BAD_RESTART"]: "a missing or wrong restart marker"}


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


class JpegCodec(Codec):
    """A level of baseline JPEG tiles.  The luma sampling ``hs, vs`` is the first parsed tile's, and every tile's after it."""
    name, tile_words, status_names = "jpeg", TILE_WORDS, STATUS_NAMES
    hs = vs = None

    def __init__(self, slide, what, compression, tags):
        super().__init__(slide, compression)
        check_samples(what, tags)
        self.transform = 1 if need_tag(what, tags, 262, (2, 6), "2 (RGB) or 6 (YCbCr) only")[0] == 6 else 0

    def attach(self, what, lv, tags):
        super().attach(what, lv, tags)
        self.base = parse_jpeg(bytes(tags[347]), what=f"{what} JPEGTables") if 347 in tags else None
        self.shared = table_set_bytes(self.base) if self.base is not None else None      # ONE object for every tile without tables of its own

    def _parse_tile(self, what, off, count):
        """offset and length: the scan's.  A tile without DQT / DHT of its own gets the level's shared table-set object
        (``self.shared``, from JPEGTables), not a copy."""
        lv = self.lv
        h = parse_jpeg(os.pread(self.slide._fd, count, off), self.base, what)
        if h.frame is None or h.scan is None:
            raise WsiFormatError(f"{what}: no SOF0 / SOS in the tile's stream")
        if (h.frame[3], h.frame[2]) != (lv.tile_w, lv.tile_h):
            raise WsiFormatError(f"{what}: SOF0 frame of {h.frame[3]} x {h.frame[2]} pixels in tiles of {lv.tile_w} x {lv.tile_h}: they must be equal")
        hs, vs = _sampling(h.frame, what)
        if self.hs is None:
            self.hs, self.vs = hs, vs
        elif (hs, vs) != (self.hs, self.vs):
            raise WsiFormatError(f"{what}: SOF0 luma sampling {hs}x{vs} where the level's first tile has {self.hs}x{self.vs}")
        sel = selectors(h, what)
        tables = self.shared if (self.shared is not None and not h.own_tables) else table_set_bytes(h)
        got = TileInfo(off + h.scan_start, h.scan_end - h.scan_start, tables, h.restart, sel)
        if got.length < 1:
            raise WsiFormatError(f"{what}: an empty entropy-coded segment")
        return got

    def table_row(self, at, info, set_index):
        return (at, info.length, set_index, info.restart, info.selectors, 0, 0, 0)

    def chunk_tile_bytes(self, L):
        """The device bytes one more tile adds to a chunk: what cuts a batch into chunks."""
        lv = self.lv
        return L.sq_jpeg_workspace_bytes(2, 1, lv.tile_w, lv.tile_h, self.hs, self.vs) - L.sq_jpeg_workspace_bytes(1, 1, lv.tile_w, lv.tile_h, self.hs, self.vs) \
            + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, self.hs, self.vs) + int(lv.counts.max())

    def decode(self, dev, blob, head, o_sets, scans_bytes, n, sets, planes, status):
        """Launch the decode of the n tiles of `blob` (tile table at 0, table sets at `o_sets`, scans at `head`) into `planes`."""
        import torch
        L = _lib.lib()
        if self.slide.entropy == "split":
            need = _lib.need(L.sq_jpeg_split_workspace_bytes, n, len(sets), *self.geom)
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)      # in the argument list: sub_bytes stands behind the workspace pair
            _lib.call("sq_jpeg_decode_tiles_split", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), *self.geom, planes, status,
                      scratch, need, self.slide.sub_bytes)
        else:
            need = _lib.need(L.sq_jpeg_workspace_bytes, n, len(sets), *self.geom)
            _lib.call("sq_jpeg_decode_tiles", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), *self.geom, planes, status, workspace=need)

    def job_extras(self, sets):
        """``tile_job``'s keys beyond the shared ones: ``transform`` and ``sets`` (the distinct table-set byte strings)."""
        return dict(transform=self.transform, sets=sets)
