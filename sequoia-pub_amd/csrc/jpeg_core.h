// Baseline-JPEG decode core shared by the device kernels (jpegdec.hip) and the host check program
// (tools/jpegdec_hostcheck.cpp): bit reader, Huffman table derivation and symbol decode, block decode, and the three integer
// stages behind it -- libjpeg's "islow" IDCT, its "fancy" chroma upsampling and its YCbCr -> RGB transform -- as
// include/sequoia_hip.h ("JPEG tiles") specifies them.  Everything is integer; products that a damaged stream can drive out
// of 32 bits are formed in uint32_t (wrapping, defined), never in int32_t.  Nothing here reads outside what it is handed:
// every byte fetch is compared with the scan's end, every table index with its extent, and no loop's trip count depends on
// stream content without a bound (<= 8 per fill, 7 per slow symbol, 63 per block, the MCU count of the frame per scan).
// The range table of libjpeg wraps rather than clamps for |v| beyond about 512 after the IDCT; no encoder of 8-bit images
// produces such values, and this core clamps.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/sequoia_hip.h"

#if defined(__HIPCC__)
#define SQJ_HD __host__ __device__ static __forceinline__
#else
#define SQJ_HD static inline
#endif

#define SQJ_LOOK 9                       // bits of the look-ahead table
#define SQJ_QUANT_BYTES 512              // 4 tables x 64 uint16, zigzag order
#define SQJ_HUFF_BYTES 272               // 16 counts + 256 symbols; tables DC0, DC1, AC0, AC1

// one derived Huffman table: look-ahead entries (length << 8 | symbol, 0: longer than SQJ_LOOK bits) and the slow path
struct SqjHuff {
    uint16_t lut[1 << SQJ_LOOK];
    int32_t maxcode[17];                 // [l]: largest code of length l, -1 when there is none
    int32_t valoff[17];                  // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
    int32_t ok;                          // 0: the table was refused (sqj_build_huff)
    int32_t pad[3];
};

struct SqjGeom {                         // one frame: three components, chroma 1 x 1, luma hs x vs
    int tile_w, tile_h, hs, vs;
    int mcus_x, mcus_y;                  // MCUs of hs * 8 x vs * 8 pixels
    int cw, ch;                          // chroma plane extent
    int blocks;                          // 8 x 8 blocks of the frame
    int plane_bytes;                     // Y plane then Cb then Cr, dense
};

SQJ_HD bool sqj_geom(int tile_w, int tile_h, int hs, int vs, SqjGeom* g) {
    if (tile_w < 16 || tile_w > SQ_JPEG_MAX_TILE || tile_h < 16 || tile_h > SQ_JPEG_MAX_TILE || (tile_w & 15) || (tile_h & 15)) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    g->tile_w = tile_w; g->tile_h = tile_h; g->hs = hs; g->vs = vs;
    g->mcus_x = tile_w / (8 * hs); g->mcus_y = tile_h / (8 * vs);
    g->cw = tile_w / hs; g->ch = tile_h / vs;
    g->blocks = (tile_w / 8) * (tile_h / 8) + 2 * (g->cw / 8) * (g->ch / 8);
    g->plane_bytes = tile_w * tile_h + 2 * g->cw * g->ch;
    return true;
}

// natural index of the k-th coefficient of the scan; the device keeps a copy in LDS (a per-lane index into constant memory is a
// global load in the middle of every coefficient)
#define SQJ_ZIGZAG_INIT {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
SQJ_HD int sqj_zigzag(int k) {
    const uint8_t zz[64] = SQJ_ZIGZAG_INIT;
    return zz[k & 63];
}

// counts[16], symbols[256] -> derived table.  Refused (false, h->ok = 0): more than 256 symbols, a length whose codes do not
// fit it with the all-ones code left free (libjpeg's rule), a DC symbol above 15.
SQJ_HD bool sqj_build_huff(const uint8_t* counts_and_vals, bool is_dc, SqjHuff* h) {
    for (int i = 0; i < (1 << SQJ_LOOK); i++) h->lut[i] = 0;
    for (int i = 0; i < 256; i++) h->vals[i] = counts_and_vals[16 + i];
    h->ok = 0;
    h->maxcode[0] = -1; h->valoff[0] = 0;
    int code = 0, p = 0;
    bool ok = true;
    for (int l = 1; l <= 16; l++) {
        const int n = counts_and_vals[l - 1];
        h->maxcode[l] = -1; h->valoff[l] = 0;
        if (ok && n) {
            if (p + n > 256 || code + n >= (1 << l)) ok = false;
            else {
                h->valoff[l] = p - code;
                h->maxcode[l] = code + n - 1;
                if (l <= SQJ_LOOK)
                    for (int i = 0; i < n; i++) {
                        const int first = (code + i) << (SQJ_LOOK - l);
                        for (int j = 0; j < (1 << (SQJ_LOOK - l)); j++) h->lut[first + j] = (uint16_t)((l << 8) | h->vals[p + i]);
                    }
                p += n; code += n;
            }
        }
        code <<= 1;
    }
    if (ok && is_dc)
        for (int i = 0; i < p; i++) ok = ok && h->vals[i] <= 15;
    h->ok = ok ? 1 : 0;
    return ok;
}

// ---- bit reader over a byte range of a 16-byte aligned buffer whose size is a multiple of 16 (little-endian) ----
struct alignas(16) SqjChunk { uint64_t lo, hi; };     // bytes come 16 at a time: one global_load_dwordx4 per 16 bytes of scan
struct SqjBits {
    const SqjChunk* words;
    SqjChunk cur;                        // the chunk at cur_at, kept across fills
    uint32_t cur_at;
    uint32_t pos, end;                   // byte positions in the buffer; pos <= end always
    uint64_t acc;
    int nbits, nreal;                    // bits in acc; how many of them came from the stream (the rest are zero fill)
    int stopped;                         // a marker or the end was met: nothing more is fetched until a restart is taken
};

SQJ_HD uint32_t sqj_chunk_byte(const SqjChunk& c, uint32_t p) { return (uint32_t)(((p & 8) ? c.hi : c.lo) >> (8 * (p & 7))) & 255u; }
SQJ_HD uint32_t sqj_byte(const SqjBits* b, uint32_t p) { return sqj_chunk_byte((p >> 4) == b->cur_at ? b->cur : b->words[p >> 4], p); }

SQJ_HD void sqj_bits_init(SqjBits* b, const SqjChunk* words, uint32_t pos, uint32_t end) {
    b->words = words; b->pos = pos; b->end = end; b->acc = 0; b->nbits = 0; b->nreal = 0; b->stopped = 0;
    b->cur_at = 0xFFFFFFFFu; b->cur.lo = 0; b->cur.hi = 0;
}

SQJ_HD void sqj_fill(SqjBits* b) {       // at least 57 bits in acc afterwards; FF 00 -> FF, a marker or the end -> zeros
    while (b->nbits <= 56) {
        uint32_t v = 0;
        if (!b->stopped) {
            if (b->pos < b->end) {
                if ((b->pos >> 4) != b->cur_at) { b->cur_at = b->pos >> 4; b->cur = b->words[b->cur_at]; }
                v = sqj_chunk_byte(b->cur, b->pos);
                if (v == 0xFF) {
                    const uint32_t next = b->pos + 1 < b->end ? sqj_byte(b, b->pos + 1) : 1u;
                    if (next == 0) b->pos += 2;
                    else { b->stopped = 1; v = 0; }
                } else b->pos += 1;
            } else b->stopped = 1;
        }
        b->acc = (b->acc << 8) | v;
        b->nbits += 8;
        if (!b->stopped) b->nreal += 8;
    }
}

SQJ_HD uint32_t sqj_peek(const SqjBits* b, int n) { return (uint32_t)(b->acc >> (b->nbits - n)) & ((1u << n) - 1u); }
SQJ_HD bool sqj_skip(SqjBits* b, int n) { b->nbits -= n; b->nreal -= n; return b->nreal >= 0; }      // false: the stream ended

// one symbol; SQ_JPEG_OK and *sym, or SQ_JPEG_BAD_CODE / SQ_JPEG_TRUNCATED.  Needs sqj_fill before it.
SQJ_HD int sqj_symbol(SqjBits* b, const SqjHuff* h, int* sym) {
    const uint32_t e = h->lut[sqj_peek(b, SQJ_LOOK)];
    if (e) {
        *sym = (int)(e & 255u);
        return sqj_skip(b, (int)(e >> 8)) ? SQ_JPEG_OK : SQ_JPEG_TRUNCATED;
    }
    const int32_t code16 = (int32_t)sqj_peek(b, 16);
    for (int l = SQJ_LOOK + 1; l <= 16; l++) {
        const int32_t code = code16 >> (16 - l);
        if (code <= h->maxcode[l]) {
            const int32_t at = code + h->valoff[l];
            if (at < 0 || at > 255) return SQ_JPEG_BAD_CODE;
            *sym = h->vals[at];
            return sqj_skip(b, l) ? SQ_JPEG_OK : SQ_JPEG_TRUNCATED;
        }
    }
    return b->nreal < 16 ? SQ_JPEG_TRUNCATED : SQ_JPEG_BAD_CODE;
}

SQJ_HD int sqj_extend(int v, int s) { return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1; }

// One 8 x 8 block: the DC difference onto *pred, the AC coefficients at their natural positions of `out` (int16 [64], which
// the caller has zeroed; only non-zero positions are written, so no per-lane array is indexed at run time).
SQJ_HD int sqj_block(SqjBits* b, const SqjHuff* dc, const SqjHuff* ac, const uint8_t* zigzag, int32_t* pred, int16_t* out) {
    int s = 0, rc;
    sqj_fill(b);
    if ((rc = sqj_symbol(b, dc, &s)) != SQ_JPEG_OK) return rc;
    if (s > 15) return SQ_JPEG_BAD_CODE;
    if (s) {
        const int v = (int)sqj_peek(b, s);
        if (!sqj_skip(b, s)) return SQ_JPEG_TRUNCATED;
        *pred += sqj_extend(v, s);
    }
    out[0] = (int16_t)(uint16_t)(uint32_t)*pred;
    for (int k = 1; k < 64; k++) {
        sqj_fill(b);
        if ((rc = sqj_symbol(b, ac, &s)) != SQ_JPEG_OK) return rc;
        const int r = s >> 4;
        s &= 15;
        if (s == 0) {
            if (r != 15) break;
            k += 15;
            continue;
        }
        k += r;
        if (k > 63) return SQ_JPEG_BAD_COEF;
        const int v = (int)sqj_peek(b, s);
        if (!sqj_skip(b, s)) return SQ_JPEG_TRUNCATED;
        out[zigzag[k]] = (int16_t)sqj_extend(v, s);
    }
    return SQ_JPEG_OK;
}

// index of block (bx, by) of component c in a tile's coefficient array (Y blocks row-major, then Cb, then Cr)
SQJ_HD int sqj_block_index(const SqjGeom* g, int c, int bx, int by) {
    const int yb = (g->tile_w / 8) * (g->tile_h / 8), cb = (g->cw / 8) * (g->ch / 8);
    return c == 0 ? by * (g->tile_w / 8) + bx : yb + (c - 1) * cb + by * (g->cw / 8) + bx;
}

// the blocks of component c in MCU (mx, my)
SQJ_HD int sqj_mcu_component(SqjBits* b, const SqjGeom* g, const SqjHuff* huff, const uint8_t* zigzag, int sel, int c, int mx, int my,
                             int32_t* pred, int16_t* coefs) {
    const int h = c == 0 ? g->hs : 1, v = c == 0 ? g->vs : 1;
    const SqjHuff* dc = huff + ((sel >> (4 * c + 2)) & 1);
    const SqjHuff* ac = huff + 2 + ((sel >> (4 * c + 3)) & 1);
    for (int j = 0; j < v; j++)
        for (int i = 0; i < h; i++) {
            const int rc = sqj_block(b, dc, ac, zigzag, pred, coefs + (size_t)sqj_block_index(g, c, mx * h + i, my * v + j) * 64);
            if (rc != SQ_JPEG_OK) return rc;
        }
    return SQ_JPEG_OK;
}

// The interleaved scan of one tile: bytes [pos, end) of `words` -> coefs int16 [g->blocks][64] (zeroed by the caller).
// sel: component c's tables at bits 4c: quantisation table (2 bits, used by the IDCT), DC table (1 bit), AC table (1 bit).
// huff: the four derived tables DC0, DC1, AC0, AC1 of the tile's table set; zigzag: the 64 entries of SQJ_ZIGZAG_INIT.
SQJ_HD int sqj_scan(const SqjChunk* words, uint32_t pos, uint32_t end, const SqjGeom* g, const SqjHuff* huff, const uint8_t* zigzag, int sel,
                    int restart, int16_t* coefs) {
    SqjBits b;
    sqj_bits_init(&b, words, pos, end);
    int32_t pred0 = 0, pred1 = 0, pred2 = 0;
    const int n_mcu = g->mcus_x * g->mcus_y;
    int mx = 0, my = 0;
    for (int n = 0; n < n_mcu; n++) {
        if (restart > 0 && n > 0 && n % restart == 0) {
            // the partial byte goes; whole unread bytes in front of the marker mean the interval was short of data
            sqj_fill(&b);
            if (b.nreal >= 8 || !b.stopped || b.pos + 2 > b.end) return b.pos + 2 > b.end ? SQ_JPEG_TRUNCATED : SQ_JPEG_BAD_RESTART;
            if (sqj_byte(&b, b.pos) != 0xFF || sqj_byte(&b, b.pos + 1) != (uint32_t)(0xD0 + ((n / restart - 1) & 7))) return SQ_JPEG_BAD_RESTART;
            sqj_bits_init(&b, words, b.pos + 2, end);
            pred0 = pred1 = pred2 = 0;
        }
        // the three components written out, so that each predictor stays a register (no pointer chosen at run time)
        int rc = sqj_mcu_component(&b, g, huff, zigzag, sel, 0, mx, my, &pred0, coefs);
        if (rc == SQ_JPEG_OK) rc = sqj_mcu_component(&b, g, huff, zigzag, sel, 1, mx, my, &pred1, coefs);
        if (rc == SQ_JPEG_OK) rc = sqj_mcu_component(&b, g, huff, zigzag, sel, 2, mx, my, &pred2, coefs);
        if (rc != SQ_JPEG_OK) return rc;
        if (++mx == g->mcus_x) { mx = 0; my++; }
    }
    return SQ_JPEG_OK;
}

// ---- one scan split over the lanes of a wave (include/sequoia_hip.h, "JPEG tiles, split entropy decode") ----
// The lane-level pieces of sq_jpeg_decode_tiles_split; the kernel (jpegdec.hip) and tools/jpegsplit_hostcheck.cpp drive them
// the same way, the one with wave shuffles and votes, the other with loops over 64 lanes.  Restart intervals are not handled
// here: a tile that has one takes sqj_scan.
//
// A state names a symbol boundary from which a FRESH reader reproduces the bits: `pos` is the byte the next bit lies in -- a
// byte the serial reader fetches as data, never the 00 of an FF 00 pair -- and `bit` how many of its bits are already used.
// The reader itself cannot give that position as pos * 8 - nbits: it looks up to 64 bits ahead and drops stuffed zeros as it
// goes (sqj_state_at walks back over what it fetched).  blk: the block's index within the MCU (luma blocks row-major, Cb, Cr);
// k: the next coefficient's zigzag index, 0 where the next symbol is a DC symbol.
struct SqjState { uint32_t pos; int32_t bit, blk, k, valid; };
struct SqjSubResult {
    SqjState end;                        // the first symbol boundary at or behind the subsequence's end; invalid after an error
    int32_t blocks;                      // block ends passed (before the error, if there was one)
    uint32_t dc0, dc1, dc2;              // sums of the DC differences per component, wrapping as the serial predictor's low bits do
    int32_t rc;                          // SQ_JPEG_OK or the error that stopped the lane
};

SQJ_HD bool sqj_state_same(const SqjState& a, const SqjState& b) {
    return a.valid == b.valid && (!a.valid || (a.pos == b.pos && a.bit == b.bit && a.blk == b.blk && a.k == b.k));
}

// one byte of [0, end) through a chunk the caller keeps (at: its index, 0xFFFFFFFF before the first use)
SQJ_HD uint32_t sqj_walk_byte(const SqjChunk* words, SqjChunk* c, uint32_t* at, uint32_t p) {
    if ((p >> 4) != *at) { *at = p >> 4; *c = words[*at]; }
    return sqj_chunk_byte(*c, p);
}

// Where a lane starts when nobody has told it better: the first bit of the subsequence that begins at byte `at` of the scan
// [pos, end), as if an MCU began there.  A subsequence that begins on the 00 of an FF 00 pair holds no bit of that pair.
SQJ_HD SqjState sqj_sub_guess(const SqjChunk* words, uint32_t pos, uint32_t end, uint32_t at) {
    SqjState s;
    s.pos = at < end ? at : end; s.bit = 0; s.blk = 0; s.k = 0; s.valid = 1;
    if (s.pos > pos && s.pos < end) {
        SqjChunk c; uint32_t cat = 0xFFFFFFFFu;
        c.lo = 0; c.hi = 0;
        if (sqj_walk_byte(words, &c, &cat, s.pos) == 0 && sqj_walk_byte(words, &c, &cat, s.pos - 1) == 0xFF) s.pos += 1;
    }
    return s;
}

// Stream bits from state `s` up to the subsequence's end: 8 for every byte in [s.pos, sub_end) that the reader takes as data
// (FF 00 is one; a marker or the scan's end stops the count as it stops the reader), less the bits already used.
SQJ_HD int sqj_sub_bits(const SqjChunk* words, const SqjState* s, uint32_t sub_end, uint32_t end) {
    SqjChunk c; uint32_t cat = 0xFFFFFFFFu;
    c.lo = 0; c.hi = 0;
    int bits = 0;
    uint32_t p = s->pos;
    while (p < sub_end) {                // sub_end <= end
        if (sqj_walk_byte(words, &c, &cat, p) == 0xFF) {
            if ((p + 1 < end ? sqj_walk_byte(words, &c, &cat, p + 1) : 1u) != 0) break;
            p += 2;
        } else p += 1;
        bits += 8;
    }
    return bits - s->bit;
}

// The state of reader `b`, which was started at byte `from`, after an error-free symbol: back from b->pos over as many
// fetched bytes as hold unread stream bits.  A 00 behind an FF was dropped by the reader unless the FF lies in front of `from`.
SQJ_HD void sqj_state_at(const SqjBits* b, uint32_t from, SqjState* s) {
    const int n = b->nreal > 0 ? b->nreal : 0;
    uint32_t p = b->pos;
    for (int t = (n + 7) >> 3; t > 0 && p > from; t--) {
        p -= 1;
        if (p > from && sqj_byte(b, p) == 0 && sqj_byte(b, p - 1) == 0xFF) p -= 1;
    }
    s->pos = p; s->bit = (8 - (n & 7)) & 7;
}

// index in the coefficient array of block n of the scan (MCU order); n < g->blocks
SQJ_HD int sqj_scan_block_index(const SqjGeom* g, int n) {
    const int luma = g->hs * g->vs, per = luma + 2;
    const int mcu = n / per, r = n - mcu * per;
    const int mx = mcu % g->mcus_x, my = mcu / g->mcus_x;
    if (r < luma) return sqj_block_index(g, 0, mx * g->hs + r % g->hs, my * g->vs + r / g->hs);
    return sqj_block_index(g, r - luma + 1, mx, my);
}

// One subsequence from state *st (valid): symbols are decoded while their first bit lies in front of sub_end (<= end), the
// last one may run over it.  write == false counts: block ends and DC sums into *o.  write == true also stores: block0 is the
// scan-order number of the block *st lies in, p0..p2 the predictors in front of it, and non-zero coefficients go to `coefs`
// (the tile's, zeroed) exactly as sqj_block writes them; it stops in front of block g->blocks, so nothing is stored outside
// the tile.  The symbol layer is sqj_symbol's and the block rules are sqj_block's, here one symbol at a time because a
// subsequence begins and ends inside blocks (sqj_block itself is kept as the serial kernel compiles it).
SQJ_HD void sqj_sub_run(const SqjChunk* words, uint32_t end, const SqjGeom* g, const SqjHuff* huff, const uint8_t* zigzag, int sel,
                        const SqjState* st, uint32_t sub_end, bool write, int block0, uint32_t p0, uint32_t p1, uint32_t p2,
                        int16_t* coefs, SqjSubResult* o) {
    o->end = *st; o->blocks = 0; o->dc0 = 0; o->dc1 = 0; o->dc2 = 0; o->rc = SQ_JPEG_OK;
    int budget = sqj_sub_bits(words, st, sub_end, end);
    if (budget <= 0) return;             // the symbol before ran over the whole of it, or there is no data here
    SqjBits b;
    sqj_bits_init(&b, words, st->pos, end);
    sqj_fill(&b);
    sqj_skip(&b, st->bit);
    const int luma = g->hs * g->vs, per = luma + 2;
    int blk = st->blk, k = st->k, n = block0, rc = SQ_JPEG_OK;
    int16_t* out = (write && n < g->blocks) ? coefs + (size_t)sqj_scan_block_index(g, n) * 64 : coefs;
    while (budget > 0 && !(write && n >= g->blocks)) {
        sqj_fill(&b);
        const int before = b.nbits;
        const int c = blk < luma ? 0 : blk - luma + 1;
        int s = 0;
        if (k == 0) {
            if ((rc = sqj_symbol(&b, huff + ((sel >> (4 * c + 2)) & 1), &s)) != SQ_JPEG_OK) break;
            if (s > 15) { rc = SQ_JPEG_BAD_CODE; break; }
            uint32_t diff = 0;
            if (s) {
                const int v = (int)sqj_peek(&b, s);
                if (!sqj_skip(&b, s)) { rc = SQ_JPEG_TRUNCATED; break; }
                diff = (uint32_t)sqj_extend(v, s);
            }
            if (c == 0) { o->dc0 += diff; p0 += diff; } else if (c == 1) { o->dc1 += diff; p1 += diff; } else { o->dc2 += diff; p2 += diff; }
            if (write) out[0] = (int16_t)(uint16_t)(c == 0 ? p0 : c == 1 ? p1 : p2);
            k = 1;
        } else {
            if ((rc = sqj_symbol(&b, huff + 2 + ((sel >> (4 * c + 3)) & 1), &s)) != SQ_JPEG_OK) break;
            const int r = s >> 4;
            s &= 15;
            if (s == 0) k = r == 15 ? k + 16 : 64;
            else {
                k += r;
                if (k > 63) { rc = SQ_JPEG_BAD_COEF; break; }
                const int v = (int)sqj_peek(&b, s);
                if (!sqj_skip(&b, s)) { rc = SQ_JPEG_TRUNCATED; break; }
                if (write) out[zigzag[k]] = (int16_t)sqj_extend(v, s);
                k += 1;
            }
        }
        if (k >= 64) {
            k = 0; n += 1; o->blocks += 1;
            blk = blk + 1 == per ? 0 : blk + 1;
            if (write && n < g->blocks) out = coefs + (size_t)sqj_scan_block_index(g, n) * 64;
        }
        budget -= before - b.nbits;
    }
    o->rc = rc;
    if (rc != SQ_JPEG_OK) { o->end.valid = 0; return; }
    sqj_state_at(&b, st->pos, &o->end);
    o->end.blk = blk; o->end.k = k; o->end.valid = 1;
}

// What a lane checks of its tile-table row before it reads a byte of the scan: SQ_JPEG_OK or the tile's status.
// huff: the derived tables of all n_sets table sets, four each.
SQJ_HD int sqj_tile_check(const int32_t* row, int n_sets, unsigned long long scans_bytes, const SqjHuff* huff) {
    const long long off = row[0], len = row[1];
    const int set = row[2], restart = row[3], sel = row[4];
    if (set < 0 || set >= n_sets) return SQ_JPEG_BAD_TABLE;
    if (off < 0 || len < 1 || (unsigned long long)(off + len) > scans_bytes || restart < 0 || (sel & ~0xFFF)) return SQ_JPEG_BAD_RANGE;
    const SqjHuff* h = huff + (size_t)set * 4;
    for (int c = 0; c < 3; c++)
        if (!h[(sel >> (4 * c + 2)) & 1].ok || !h[2 + ((sel >> (4 * c + 3)) & 1)].ok) return SQ_JPEG_BAD_TABLE;
    return SQ_JPEG_OK;
}

// ---- IDCT: libjpeg jidctint.c (islow), 13-bit constants ----
// one 1-D pass over x[0..7] (stride 1 in this array), each output (v + (1 << (n - 1))) >> n with an arithmetic shift
SQJ_HD void sqj_idct_1d(const int32_t* x, int32_t* y, int n) {
    const uint32_t x0 = (uint32_t)x[0], x1 = (uint32_t)x[1], x2 = (uint32_t)x[2], x3 = (uint32_t)x[3];
    const uint32_t x4 = (uint32_t)x[4], x5 = (uint32_t)x[5], x6 = (uint32_t)x[6], x7 = (uint32_t)x[7];
    uint32_t z1 = (x2 + x6) * 4433u;
    const uint32_t t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
    const uint32_t t0 = (x0 + x4) * 8192u, t1 = (x0 - x4) * 8192u;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = x7, b = x5, c = x3, d = x1;
    z1 = a + d;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
    const uint32_t z5 = (z3 + z4) * 9633u;
    a *= 2446u; b *= 16819u; c *= 25172u; d *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5;
    z4 = z4 * (uint32_t)-3196 + z5;
    a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
    const uint32_t r = 1u << (n - 1);
    y[0] = (int32_t)(t10 + d + r) >> n; y[7] = (int32_t)(t10 - d + r) >> n;
    y[1] = (int32_t)(t11 + c + r) >> n; y[6] = (int32_t)(t11 - c + r) >> n;
    y[2] = (int32_t)(t12 + b + r) >> n; y[5] = (int32_t)(t12 - b + r) >> n;
    y[3] = (int32_t)(t13 + a + r) >> n; y[4] = (int32_t)(t13 - a + r) >> n;
}
SQJ_HD int32_t sqj_dequant(int16_t coef, uint16_t q) { return (int32_t)((uint32_t)(int32_t)coef * (uint32_t)q); }
SQJ_HD uint8_t sqj_clamp_u8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
SQJ_HD uint8_t sqj_sample(int32_t v) { return sqj_clamp_u8(v + 128); }      // v is a 32-bit value shifted right by 18

// one block: coefficients (natural order) and its quantisation table (natural order) -> 8 x 8 samples at `out` with row `stride`:
// the column pass and then the row pass, as the device kernel runs them through LDS
SQJ_HD void sqj_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, int stride) {
    int32_t ws[64], x[8], y[8];
    for (int col = 0; col < 8; col++) {
        for (int r = 0; r < 8; r++) x[r] = sqj_dequant(coef[r * 8 + col], q[r * 8 + col]);
        sqj_idct_1d(x, y, 11);
        for (int r = 0; r < 8; r++) ws[r * 8 + col] = y[r];
    }
    for (int r = 0; r < 8; r++) {
        sqj_idct_1d(ws + r * 8, y, 18);
        for (int j = 0; j < 8; j++) out[(size_t)r * stride + j] = sqj_sample(y[j]);
    }
}

// ---- planes -> pixel: fancy upsampling of one chroma plane [ch][cw] at luma position (px, py) ----
SQJ_HD int sqj_chroma(const uint8_t* plane, const SqjGeom* g, int px, int py) {
    if (g->hs == 1) return plane[(size_t)py * g->cw + px];
    const int i = px >> 1, n = g->cw;
    if (g->vs == 1) {
        const uint8_t* row = plane + (size_t)py * n;
        if (px & 1) return i == n - 1 ? row[n - 1] : (3 * row[i] + row[i + 1] + 2) >> 2;
        return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = py >> 1;
    int fr = (py & 1) ? r + 1 : r - 1;
    fr = fr < 0 ? 0 : fr > g->ch - 1 ? g->ch - 1 : fr;
    const uint8_t* near_row = plane + (size_t)r * n;
    const uint8_t* far_row = plane + (size_t)fr * n;
    const int cs = 3 * near_row[i] + far_row[i];
    if (px & 1) return i == n - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * near_row[i + 1] + far_row[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * near_row[i - 1] + far_row[i - 1] + 8) >> 4;
}

// pixel (px, py) of a tile's planes as R | G << 8 | B << 16 | 255 << 24; transform: YCbCr -> RGB (photometric 6), else as stored
SQJ_HD uint32_t sqj_pixel(const uint8_t* planes, const SqjGeom* g, int px, int py, int transform) {
    const int y = planes[(size_t)py * g->tile_w + px];
    const uint8_t* cbp = planes + (size_t)g->tile_w * g->tile_h;
    int cb = sqj_chroma(cbp, g, px, py), cr = sqj_chroma(cbp + (size_t)g->cw * g->ch, g, px, py);
    int R = y, G = cb, B = cr;
    if (transform) {
        cb -= 128; cr -= 128;
        R = sqj_clamp_u8(y + ((91881 * cr + 32768) >> 16));
        G = sqj_clamp_u8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        B = sqj_clamp_u8(y + ((116130 * cb + 32768) >> 16));
    }
    return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16) | 0xFF000000u;
}
