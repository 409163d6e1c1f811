"""LZW and uncompressed levels (compression 5 / 1: the lossless pyramids libvips, QuPath, Bio-Formats and tiffcp write; a level is one
codec): a tile is chunky RGB of 8 bits, decoded by ``sq_lzw_decode_tiles`` (csrc/tifflzw.hip, csrc/lzw_core.h) into the same planes,
every byte libtiff's.  Accepted: photometric 2 (RGB), three samples of 8 bits, planar configuration 1, FillOrder absent or 1,
Predictor absent, 1 or 2 (horizontal differencing, undone on the device), the tile extents every level has (package
docstring); LZW streams MSB first with libtiff's early change, opening with the Clear code.  Refused by name: Predictor 3, ExtraSamples or four samples (RGBA), FillOrder
2, any other photometric, an uncompressed tile whose byte count is not tile width x height x 3, old-style LZW (LSB first, no
Clear at the start); deflate (8, 32946) and every other compression.  A stream that overruns the code table without a Clear is
refused where libtiff refuses it, when the tile is read (``TileDecodeError``)."""
import os

import numpy as np

from . import WsiFormatError
from .. import _lib
from .._abi import CONSTANTS as _C
from .tiff import Codec, TileInfo, _one, check_samples

LZW_TILE_WORDS = _C["SQ_LZW_TILE_WORDS"]
LZW_STATUS_NAMES = {_C["SQ_LZW_BAD_RANGE"]: "a tile range outside the uploaded bytes",
                    _C["SQ_LZW_TRUNCATED"]: "the tile's bytes end before the tile is full",
                    _C["SQ_LZW_BAD_CODE"]: "an LZW code above the next free table entry",
                    _C["SQ_LZW_NO_CLEAR"]: "an LZW stream that does not start with the Clear code",
                    _C["SQ_LZW_TABLE_FULL"]: "an LZW stream that overruns the code table without a Clear code",
                    _C["SQ_LZW_EARLY_EOI"]: "the LZW end-of-information code before the tile is full"}
LZW_COMPRESSIONS = {5: "LZW", 1: "uncompressed"}
LZW_MODE = _C["SQ_LZW_MODE_WAVE"]         # SQ_LZW_MODE_WAVE: a wave per tile; SQ_LZW_MODE_LANE: a lane per tile, the serial reference


class LosslessCodec(Codec):
    """A level of LZW ('lzw') or uncompressed ('raw') tiles: chunky RGB as stored, so no colour transform, no subsampling, no
    alpha, and no table sets -- the predictor is all a tile needs besides its bytes."""
    tile_words, status_names = LZW_TILE_WORDS, LZW_STATUS_NAMES

    def __init__(self, slide, what, compression, tags):
        super().__init__(slide, compression)
        self.name = "lzw" if compression == 5 else "raw"
        what_comp = f"{what}: Compression = {compression} ({LZW_COMPRESSIONS[compression]})"
        if _one(tags, 262) != 2:
            raise WsiFormatError(f"{what_comp} with PhotometricInterpretation = {_one(tags, 262)}: 2 (RGB) only")
        if 338 in tags:
            raise WsiFormatError(f"{what_comp} with ExtraSamples = {tuple(int(x) for x in tags[338])}: three samples without alpha only")
        if _one(tags, 266, 1) != 1:
            raise WsiFormatError(f"{what_comp} with FillOrder = {_one(tags, 266)}: 1 (most significant bit first) only")
        if _one(tags, 317, 1) not in (1, 2):
            kind = " (floating point)" if _one(tags, 317) == 3 else ""
            raise WsiFormatError(f"{what_comp} with Predictor = {_one(tags, 317)}{kind}: 1 (none) or 2 (horizontal differencing) only")
        check_samples(what, tags)
        self.predictor = _one(tags, 317, 1)

    def attach(self, what, lv, tags):
        super().attach(what, lv, tags)
        if self.compression == 1 and (lv.counts != lv.tile_w * lv.tile_h * 3).any():
            t = int(np.flatnonzero(lv.counts != lv.tile_w * lv.tile_h * 3)[0])
            raise WsiFormatError(f"{what}: Compression = 1 (uncompressed) with TileByteCounts[{t}] = {int(lv.counts[t])} (tile {t % lv.tiles_x}, "
                                 f"{t // lv.tiles_x}): tiles of {lv.tile_w} x {lv.tile_h} x 3 samples hold {lv.tile_w * lv.tile_h * 3} bytes")

    def _parse_tile(self, what, off, count):
        """The whole tile is the scan; an LZW stream must open with the Clear code (256 in 9 bits)."""
        first = os.pread(self.slide._fd, 2, off)
        if self.compression == 5 and (len(first) < 2 or first[0] != 0x80 or first[1] & 0x80):
            raise WsiFormatError(f"IFD {self.lv.index}: Compression = 5 (LZW) but {what} starts with bytes {first.hex(' ')}, not with the Clear code "
                                 f"(80 00 in nine bits): old-style LZW (least significant bit first, no Clear at the start) is not supported")
        return TileInfo(off, count, b"", 0, 0)

    def chunk_tile_bytes(self, L):
        """The device bytes one more tile adds to a chunk: what cuts a batch into chunks."""
        lv = self.lv
        return L.sq_lzw_workspace_bytes(2, lv.tile_w, lv.tile_h, self.compression) - L.sq_lzw_workspace_bytes(1, lv.tile_w, lv.tile_h, self.compression) \
            + L.sq_jpeg_planes_bytes(1, lv.tile_w, lv.tile_h, 1, 1) + int(lv.counts.max())

    def decode(self, dev, blob, head, o_sets, scans_bytes, n, sets, planes, status):
        """Launch the decode of the n tiles of `blob` (tile table at 0, the tiles' bytes at `head`) into `planes`, in the
        slide's ``lzw_mode`` as it stands at the call (None: ``LZW_MODE``; no CLI sets it)."""
        lv = self.lv
        mode = LZW_MODE if self.slide.lzw_mode is None else self.slide.lzw_mode
        need = _lib.need(_lib.lib().sq_lzw_workspace_bytes, n, lv.tile_w, lv.tile_h, self.compression)
        _lib.call("sq_lzw_decode_tiles", dev, blob[head:], scans_bytes, blob, n, lv.tile_w, lv.tile_h, self.compression, self.predictor, mode,
                  planes, status, workspace=need)

    def job_extras(self, sets):
        """``tile_job``'s key beyond the shared ones: ``predictor``; there are no sets."""
        return dict(predictor=self.predictor)
