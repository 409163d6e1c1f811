"""Cases, fixture writer and numpy restatement for the JPEG-tiled TIFF / SVS reader (sequoia_pub_amd.wsi, csrc/jpegdec.hip).

``CASES`` lists the fixture files under tests/golden/wsi/ (made by tests/golden/make_wsi_golden.py with Pillow: the compressed
.tif files and wsi.npz with Pillow's decoded bytes of every level and of every stand-alone tile stream).  ``write_tiff`` is a
small classic / BigTIFF writer for fixtures only.  ``decode_tile`` restates the arithmetic of include/sequoia_hip.h ("JPEG
tiles") in numpy and pure Python, independently of csrc/jpeg_core.h, and counts the events (FF 00 stuffing, zero-run symbols,
codes beyond the look-ahead) the noise case must keep covering."""
import os
import struct

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wsi")
APERIO = "Aperio Image Library v12.0.15\r\n{w}x{h} [0,0 {w}x{h}] ({t}x{t}) JPEG/RGB Q={q}|AppMag = 20|MPP = 0.5021|Filename = synthetic"

# name -> levels [(width, height)], tile, subsampling (Pillow: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), quality, photometric, restart
# interval in MCUs, optimize (tiles carry their own Huffman tables, no JPEGTables), bigtiff, content, stripped IFDs interleaved
CASES = {
    "ycc420":   dict(levels=[(150, 100), (75, 50)], tile=32, subsampling=2, quality=75, photometric=6, restart=0, optimize=False, bigtiff=False, content="smooth", stripped=True),
    "ycc422":   dict(levels=[(150, 100), (75, 50)], tile=32, subsampling=1, quality=60, photometric=6, restart=2, optimize=False, bigtiff=False, content="smooth", stripped=False),
    "ycc444":   dict(levels=[(150, 100), (75, 50)], tile=32, subsampling=0, quality=90, photometric=6, restart=3, optimize=False, bigtiff=False, content="smooth", stripped=False),
    "big420":   dict(levels=[(150, 100), (75, 50)], tile=32, subsampling=2, quality=75, photometric=6, restart=0, optimize=False, bigtiff=True, content="smooth", stripped=True, like="ycc420"),
    "tile48":   dict(levels=[(100, 70)], tile=48, subsampling=1, quality=20, photometric=6, restart=0, optimize=False, bigtiff=False, content="smooth", stripped=False),
    "single16": dict(levels=[(16, 16)], tile=16, subsampling=2, quality=95, photometric=6, restart=0, optimize=False, bigtiff=False, content="flat", stripped=False),
    "rgb444":   dict(levels=[(70, 40)], tile=32, subsampling=0, quality=80, photometric=2, restart=0, optimize=False, bigtiff=False, content="smooth", stripped=False),
    "optimize": dict(levels=[(70, 40)], tile=32, subsampling=2, quality=85, photometric=6, restart=0, optimize=True, bigtiff=True, content="smooth", stripped=False),
    "noise100": dict(levels=[(96, 32)], tile=32, subsampling=0, quality=100, photometric=6, restart=0, optimize=False, bigtiff=False, content="noise", stripped=False),
}
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}
# the synthetic slide of the pipeline tests: the smallest the patch filter admits (256-pixel regions)
PIPELINE = dict(levels=[(1024, 768), (128, 96)], tile=256, subsampling=1, quality=70, photometric=6, restart=0, optimize=False, bigtiff=False,
                content="tissue", stripped=True)


def level_image(content, width, height, seed):
    """uint8 [height, width, 3] of one level."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    if content == "flat":
        return np.broadcast_to(np.array([180, 90, 140], dtype=np.uint8), (height, width, 3)).copy()
    if content == "noise":       # uniform noise, and on the right 32 columns grey blocks of two high frequencies (long zero runs)
        img = rng.randint(0, 256, size=(height, width, 3)).astype(np.uint8)
        k = np.arange(8)
        wave = np.outer(np.cos((2 * k + 1) * 7 * np.pi / 16), np.cos((2 * k + 1) * 6 * np.pi / 16))
        block = np.rint(128 + 30 * wave + 20 * wave.T[::-1]).astype(np.uint8)
        img[:, width - 32:] = np.tile(block, (height // 8 + 1, 4))[:height, :, None]
        return img
    if content == "smooth":
        img = np.stack([128 + 100 * np.sin(x / 9.0 + seed) * np.cos(y / 13.0), 128 + 110 * np.cos(x / 17.0 - y / 7.0),
                        40 + 1.3 * x + 0.6 * y], -1)
        img[height // 3:height // 3 + 9, width // 4:width // 4 + 21] = (250, 20, 30)          # hard edges: high frequencies
        return np.clip(img + rng.randint(-6, 7, size=img.shape), 0, 255).astype(np.uint8)
    if content == "tissue":      # blocks of 16 x 16 pixels from a small palette: pink tissue with contrast on white glass
        by, bx = (height + 15) // 16, (width + 15) // 16
        palette = np.array([[236, 236, 236], [200, 110, 170], [150, 60, 130], [225, 160, 200], [110, 40, 100]], dtype=np.uint8)
        cy, cx = np.mgrid[0:by, 0:bx]
        inside = ((cx - bx * 0.45) ** 2 / (bx * 0.36) ** 2 + (cy - by * 0.5) ** 2 / (by * 0.40) ** 2) < 1.0
        idx = np.where(inside, 1 + rng.randint(0, 4, size=(by, bx)), 0)
        return np.repeat(np.repeat(palette[idx], 16, 0), 16, 1)[:height, :width].copy()
    raise ValueError(content)


def case_levels(name):
    """The level images of a case: level i > 0 is level 0 decimated (any content serves: every level is compared on its own)."""
    spec = PIPELINE if name == "pipeline" else CASES[name]
    w0, h0 = spec["levels"][0]
    base = level_image(spec["content"], w0, h0, seed=sum(map(ord, spec.get("like", name))) % 1000)
    out = [base]
    for w, h in spec["levels"][1:]:
        ys, xs = (np.arange(h) * h0) // h, (np.arange(w) * w0) // w
        out.append(base[ys][:, xs].copy())
    return out


# ---- TIFF writer (fixtures only) -------------------------------------------------------------------------------------------
def write_tiff(path, ifds, bigtiff=False, byteorder="<"):
    """ifds: list of dicts tag -> (type, values); type 2 / 7 take bytes.  A tag 324 / 273 given as a list of byte strings is the
    tile / strip data: the writer lays the data out and fills the offsets, with the byte counts under tag + 1 (325) or 279."""
    bo = byteorder
    fmt = {1: "B", 2: "s", 3: "H", 4: "I", 7: "s", 16: "Q"}
    off_t, off_fmt, inline = (16, "Q", 8) if bigtiff else (4, "I", 4)
    out = bytearray(struct.pack(bo + "2sHHHQ", b"II" if bo == "<" else b"MM", 43, 8, 0, 0) if bigtiff else
                    struct.pack(bo + "2sHI", b"II" if bo == "<" else b"MM", 42, 0))
    link_at = 8 if bigtiff else 4
    for tags in ifds:
        tags = dict(tags)
        for data_tag, count_tag in ((324, 325), (273, 279)):
            if data_tag in tags and isinstance(tags[data_tag], list):
                offsets = []
                for blob in tags[data_tag]:
                    offsets.append(len(out))
                    out += blob + b"\0" * (len(out) + len(blob) & 1)
                tags[count_tag] = (off_t, [len(b) for b in tags[data_tag]])
                tags[data_tag] = (off_t, offsets)
        entries = []
        for tag in sorted(tags):
            kind, values = tags[tag]
            if kind in (2, 7):
                raw, count = bytes(values), len(values)
            else:
                values = list(values) if isinstance(values, (list, tuple)) else [values]
                raw, count = struct.pack(bo + fmt[kind] * len(values), *values), len(values)
            if len(raw) > inline:
                if len(out) & 1:
                    out += b"\0"
                at = len(out)
                out += raw
                raw = struct.pack(bo + off_fmt, at)
            entries.append(struct.pack(bo + ("HHQ8s" if bigtiff else "HHI4s"), tag, kind, count, raw.ljust(inline, b"\0")))
        if len(out) & 1:
            out += b"\0"
        struct.pack_into(bo + off_fmt, out, link_at, len(out))
        out += struct.pack(bo + ("Q" if bigtiff else "H"), len(entries)) + b"".join(entries)
        link_at = len(out)
        out += struct.pack(bo + off_fmt, 0)
    with open(path, "wb") as f:
        f.write(out)


def level_ifd(width, height, tile, tile_streams, photometric, subsampling, tables=None, description=None, compression=7):
    hs, vs = SAMPLING[subsampling]
    tags = {256: (4, width), 257: (4, height), 258: (3, [8, 8, 8]), 259: (3, compression), 262: (3, photometric), 277: (3, 3), 284: (3, 1),
            322: (4, tile), 323: (4, tile), 324: list(tile_streams)}
    if photometric == 6:
        tags[530] = (3, [hs, vs])
    if tables is not None:
        tags[347] = (7, tables)
    if description is not None:
        tags[270] = (2, description.encode() + b"\0")
    return tags


def stripped_ifd(width, height):
    """An uncompressed RGB strip image (the thumbnail / label / macro of an SVS): never a level."""
    data = np.full((height, width, 3), 200, dtype=np.uint8).tobytes()
    return {256: (4, width), 257: (4, height), 258: (3, [8, 8, 8]), 259: (3, 1), 262: (3, 2), 277: (3, 3), 278: (4, height), 284: (3, 1),
            273: [data]}


def pad_tile(img, tx, ty, tile):
    """Tile (tx, ty) of a level image, its part beyond the level replicated from the edge."""
    h, w = img.shape[:2]
    ys = np.minimum(np.arange(ty * tile, (ty + 1) * tile), h - 1)
    xs = np.minimum(np.arange(tx * tile, (tx + 1) * tile), w - 1)
    return img[ys][:, xs]


# ---- numpy restatement of the decode (include/sequoia_hip.h, "JPEG tiles") ---------------------------------------------------
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def parse_stream(data):
    """Marker segments of a full stream -> (quant {id: int[64] zigzag}, huff {(class, id): {(length, code): symbol}}, frame
    (height, width, [(id, h, v, tq)]), scan [(id, td, ta)], restart interval, scan bytes)."""
    quant, huff, frame, restart, pos = {}, {}, None, 0, 2
    while True:
        assert data[pos] == 0xFF, (pos, data[pos])
        m, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg, end = pos + 4, pos + 2 + length
        if m == 0xDB:
            while seg < end:
                pq, tq = data[seg] >> 4, data[seg] & 15
                step = 2 if pq else 1
                quant[tq] = [int.from_bytes(data[seg + 1 + step * i:seg + 1 + step * (i + 1)], "big") for i in range(64)]
                seg += 1 + 64 * step
        elif m == 0xC4:
            while seg < end:
                tc, th = data[seg] >> 4, data[seg] & 15
                counts = data[seg + 1:seg + 17]
                codes, code, at = {}, 0, seg + 17
                for length_bits in range(1, 17):
                    for _ in range(counts[length_bits - 1]):
                        codes[(length_bits, code)] = data[at]
                        code += 1
                        at += 1
                    code <<= 1
                huff[(tc, th)] = codes
                seg = at
        elif m == 0xC0:
            frame = ((data[seg + 1] << 8) | data[seg + 2], (data[seg + 3] << 8) | data[seg + 4],
                     [(data[seg + 6 + 3 * i], data[seg + 7 + 3 * i] >> 4, data[seg + 7 + 3 * i] & 15, data[seg + 8 + 3 * i]) for i in range(data[seg + 5])])
        elif m == 0xDD:
            restart = (data[seg] << 8) | data[seg + 1]
        elif m == 0xDA:
            scan = [(data[seg + 1 + 2 * i], data[seg + 2 + 2 * i] >> 4, data[seg + 2 + 2 * i] & 15) for i in range(data[seg])]
            stop = data.rfind(b"\xff\xd9", end)
            return quant, huff, frame, scan, restart, data[end:stop if stop >= 0 else len(data)]
        else:
            assert m not in (0xC1, 0xC2, 0xC9, 0xCA), f"frame marker {m:#x}"
        pos = end


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.acc, self.n, self.stuffed = data, 0, 0, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.data[self.pos] == 0, "marker inside an interval"
                self.pos += 1
                self.stuffed += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in codes:
                return codes[(length, code)], length
        raise AssertionError("a code that matches no table entry")


def _extend(v, s):
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _idct_pass(x, n):
    """One 1-D pass over the LAST axis of an int64 array [..., 8]."""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
    z1 = (x2 + x6) * 4433
    t2, t3 = z1 - x6 * 15137, z1 + x2 * 6270
    t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x7, x5, x3, x1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], -1)
    return (out + (1 << (n - 1))) >> n


def _upsample(plane, hs, vs):
    p = plane.astype(np.int64)
    if hs == 1:
        return p
    if vs == 2:
        up, down = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
        rows = np.empty((2 * p.shape[0], p.shape[1]), dtype=np.int64)
        rows[0::2], rows[1::2] = 3 * p + up, 3 * p + down
        left, right = np.hstack([rows[:, :1], rows[:, :-1]]), np.hstack([rows[:, 1:], rows[:, -1:]])
        out = np.empty((rows.shape[0], 2 * rows.shape[1]), dtype=np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
        return out
    left, right = np.hstack([p[:, :1], p[:, :-1]]), np.hstack([p[:, 1:], p[:, -1:]])
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def decode_tile(stream, transform, events=None):
    """A full baseline stream (tables joined in front where they are shared) -> uint8 [H, W, 3].  ``events``: a dict that
    receives the counts of FF 00 pairs, zero-run (ZRL) symbols and codes of more than 9 bits."""
    quant, huff, (height, width, comps), scan, restart, data = parse_stream(stream)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    tables = {cid: (td, ta) for cid, td, ta in scan}
    coefs = [np.zeros((my * c[2], mx * c[1], 64), dtype=np.int64) for c in comps]
    bits, pred, zrl, long_codes = _Bits(data), [0] * len(comps), 0, 0
    stuffed = 0
    for n in range(mx * my):
        if restart and n and n % restart == 0:
            stuffed += bits.stuffed
            at = bits.pos
            assert data[at] == 0xFF and data[at + 1] == 0xD0 + ((n // restart - 1) & 7), "restart marker"
            bits = _Bits(data[at + 2:])
            data = bits.data
            pred = [0] * len(comps)
        for ci, (cid, h, v, tq) in enumerate(comps):
            td, ta = tables[cid]
            for j in range(v):
                for i in range(h):
                    blk = coefs[ci][(n // mx) * v + j, (n % mx) * h + i]
                    s, length = bits.symbol(huff[(0, td)])
                    pred[ci] += _extend(bits.bits(s), s) if s else 0
                    blk[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs, length = bits.symbol(huff[(1, ta)])
                        long_codes += length > 9
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            zrl += 1
                            k += 16
                            continue
                        k += r
                        assert k <= 63, "run past coefficient 63"
                        blk[ZIGZAG[k]] = _extend(bits.bits(s), s)
                        k += 1
    if events is not None:
        events.update(stuffed=stuffed + bits.stuffed, zrl=zrl, long_codes=long_codes)
    planes = []
    for ci, (cid, h, v, tq) in enumerate(comps):
        q = np.zeros(64, dtype=np.int64)
        q[ZIGZAG] = quant[tq]
        blocks = (coefs[ci] * q).reshape(coefs[ci].shape[0], coefs[ci].shape[1], 8, 8)
        cols = _idct_pass(blocks.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns first
        pix = np.clip(_idct_pass(cols, 18) + 128, 0, 255)
        plane = pix.transpose(0, 2, 1, 3).reshape(pix.shape[0] * 8, pix.shape[1] * 8)
        planes.append(plane[:-(-height * v // vmax), :-(-width * h // hmax)])
    y = planes[0]
    cb, cr = (_upsample(p, hmax // comps[i + 1][1], vmax // comps[i + 1][2])[:height, :width] for i, p in enumerate(planes[1:]))
    if transform:
        cb, cr = cb - 128, cr - 128
        rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)]
    else:
        rgb = [y, cb, cr]
    return np.clip(np.stack(rgb, -1), 0, 255).astype(np.uint8)


def join_tables(tables, tile):
    """An abbreviated table stream and an image-only stream as one full stream."""
    return tile if tables is None else tables[:-2] + tile[2:]


# ---- the stand-alone host programs of the slide codecs (tools/*_hostcheck.cpp) ------------------------------------------------
def build_hostcheck(source, directory, sanitize, extra_flags=()):
    """tools/`source` built with the host compiler into `directory`; returns a runner ``run(jobs, *args)`` over a job directory
    that asserts a clean exit (and, with `sanitize`, a clean address / undefined-behaviour sanitizer run) and gives the output."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, f"no host C++ compiler (c++, g++ or clang++) to build tools/{source}"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(directory), os.path.splitext(source)[0] + ("_san" if sanitize else ""))
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra_flags, *flags, "-o", exe, os.path.join(root, "tools", source)], check=True)

    def run(jobs, *args):
        r = subprocess.run([exe, str(jobs), *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
        return r.stdout
    return run


# ---- what read_regions uploads, as recorded results (tests/golden/wsi_jobs.json) -----------------------------------------------
JOBS_GOLDEN = os.path.join(os.path.dirname(GOLDEN_DIR), "wsi_jobs.json")
JOBS_GOLDEN_DIRS = ("wsi", "j2k", "tiffz")


def job_fixtures():
    """'<directory>/<name>' of every slide fixture whose upload is recorded."""
    root = os.path.dirname(GOLDEN_DIR)
    return [f"{d}/{f[:-4]}" for d in JOBS_GOLDEN_DIRS for f in sorted(os.listdir(os.path.join(root, d))) if f.endswith(".tif")]


def job_records(slide):
    """Per level of an open slide: the SHA-256 of its tile ranges, and ``tile_job`` of the whole level ('all') and of every
    second tile in descending order ('half') -- the plain values as they are, the table, the sets and the scans as SHA-256."""
    import hashlib

    def sha(data):
        return hashlib.sha256(data).hexdigest()

    def record(job):
        out = dict(codec=job["codec"], geom=[int(v) for v in job["geom"]], tiles=[int(t) for t in job["tiles"]])
        for key in ("transform", "predictor"):
            if key in job:
                out[key] = int(job[key])
        if "caps" in job:
            out["caps"] = [int(v) for v in job["caps"]]
        out["table_shape"] = list(job["table"].shape)
        out["table"] = sha(job["table"].tobytes())
        if "sets" in job:
            out["sets_count"] = len(job["sets"])
            out["sets"] = sha(b"".join(job["sets"]))
        out["scans"] = sha(job["scans"].tobytes())
        return out
    levels = []
    for level in range(slide.level_count):
        offsets, counts = slide.tile_ranges(level)
        half = sorted(range(0, len(offsets), 2), reverse=True)
        levels.append(dict(tile_ranges=sha(offsets.astype("<i8").tobytes() + counts.astype("<i8").tobytes()),
                           all=record(slide.tile_job(level)), half=record(slide.tile_job(level, tiles=half))))
    return levels
