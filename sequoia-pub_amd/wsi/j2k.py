"""JPEG 2000 levels (compression 33003 / 33005, Aperio's ``J2K/KDU``; a level is one codec): a tile is one raw codestream (SOC ... EOC, no
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
bytes are equal for reversible streams with every pass present and within 1 grey level (about 1 byte in 1000) otherwise."""
import os
import struct

import numpy as np

from . import WsiFormatError
from .. import _lib
from .._abi import CONSTANTS as _C
from .tiff import Codec, TileInfo, check_samples

J2K_TILE_WORDS = _C["SQ_J2K_TILE_WORDS"]
J2K_STATUS_NAMES = {_C["SQ_J2K_BAD_PARAM"]: "a parameter-set field out of range or a missing parameter set",
                    _C["SQ_J2K_BAD_RANGE"]: "a packet range outside the uploaded bytes",
                    _C["SQ_J2K_TRUNCATED_HEADER"]: "a packet header runs past the end of the tile's bytes",
                    _C["SQ_J2K_BAD_LENGTH"]: "a pass count, bit-plane count or length that does not fit the code-block or the stream",
                    _C["SQ_J2K_TRUNCATED_BODY"]: "the code-block bytes of a packet run past the end of the tile's bytes"}
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


class J2kCodec(Codec):
    """A level of raw JPEG 2000 codestreams.  ``caps``: per parameter set, the record counts the workspace is sized by."""
    name, tile_words, status_names = "j2k", J2K_TILE_WORDS, J2K_STATUS_NAMES

    def __init__(self, slide, what, compression, tags):
        super().__init__(slide, compression)
        check_samples(what, tags)
        self.transform = 1 if compression == 33003 else 0          # the photometric tag is not consulted
        self.caps = {}

    def _parse_tile(self, what, off, count):
        """offset and length: the packets'; tables: the parameter-set bytes."""
        lv = self.lv
        data = os.pread(self.slide._fd, count, off)
        if data[:2] != b"\xff\x4f":
            found = "a JPEG stream (SOI)" if data[:2] == b"\xff\xd8" else ("a JP2 file (boxes)" if data[4:8] == b"jP  " else f"bytes {data[:4].hex(' ')}")
            raise WsiFormatError(f"IFD {lv.index}: Compression = {self.compression} ({J2K_COMPRESSIONS[self.compression]}) but {what} holds {found} "
                                 f"where a raw codestream (SOC, ff 4f) was expected")
        h = parse_j2k(data, what)
        if h.size != (lv.tile_w, lv.tile_h):
            raise WsiFormatError(f"{what}: SIZ image of {h.size[0]} x {h.size[1]} pixels in tiles of {lv.tile_w} x {lv.tile_h}: they must be equal")
        return TileInfo(off + h.body_start, h.body_end - h.body_start, h.params, 0, 0)

    def _caps(self, sets):
        """(code-blocks, tag-tree nodes, precinct-bands) a tile of `sets` (parameter-set byte strings) needs at most: the
        library's own count (sq_j2k_layout, host only), kept per set."""
        import ctypes
        for params in sets:
            if params not in self.caps:
                counts = (ctypes.c_int32 * 3)()
                _lib.check(_lib.lib().sq_j2k_layout(params, self.lv.tile_w, self.lv.tile_h, ctypes.cast(counts, ctypes.c_void_p)))
                self.caps[params] = tuple(counts)
        return tuple(max(1, max(self.caps[p][i] for p in sets)) for i in range(3))

    def chunk_tile_bytes(self, L):
        """The device bytes one more tile adds to a chunk: what cuts a batch into chunks.  The records of the first tile's
        parameter set stand for the level's in this estimate."""
        lv = self.lv
        caps = self._caps([self.tile_info(0).tables])
        return L.sq_j2k_workspace_bytes(2, lv.tile_w, lv.tile_h, *caps, 16) - L.sq_j2k_workspace_bytes(1, lv.tile_w, lv.tile_h, *caps, 16) \
            + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, 1, 1) + 2 * int(lv.counts.max())

    def decode(self, dev, blob, head, o_sets, scans_bytes, n, sets, planes, status):
        """Launch the decode of the n tiles of `blob` (tile table at 0, parameter sets at `o_sets`, packets at `head`) into `planes`."""
        lv = self.lv
        caps = self._caps(sets)
        need = _lib.need(_lib.lib().sq_j2k_workspace_bytes, n, lv.tile_w, lv.tile_h, *caps, scans_bytes)
        _lib.call("sq_j2k_decode_tiles", dev, blob[head:], scans_bytes, blob, n, blob[o_sets:], len(sets), lv.tile_w, lv.tile_h, *caps,
                  planes, status, workspace=need)

    def job_extras(self, sets):
        """``tile_job``'s keys beyond the shared ones: ``transform``, ``sets`` (the distinct parameter-set byte strings) and
        ``caps``, the record counts the workspace is sized by."""
        return dict(transform=self.transform, sets=sets, caps=self._caps(sets))
