// TIFF LZW decode core shared by the device kernels (tifflzw.hip) and the host check program (tools/lzw_hostcheck.cpp):
// where the codes of a stream lie, the serial decoder over (position, length) entries and the status rules, as
// include/sequoia_hip.h ("LZW and uncompressed tiles") specifies them.
//
// Codes are packed MSB first.  Behind a Clear the codes are numbered j = 0, 1, ...; code j >= 1 makes entry 257 + j, so the
// next free entry when code j is read is 257 + j and the width of code j (libtiff's early change: 9 bits while the next free
// entry is below 511, 10 below 1023, 11 below 2047, then 12) and its bit position are functions of j alone.  The Clear or EOI
// that ends a segment is itself read at the width of its number.
// Entry 258 + i is the string of code i followed by the first byte of the string of code i + 1: in the output those bytes lie
// next to each other, so the table holds (position of the string of code i, its length) and no bytes.  A code c >= 258 read as
// code j names i = c - 258 and is valid for i <= j - 1; its string is out[pos_i .. pos_i + len_i] (len_i + 1 bytes), and for
// i = j - 1 (the code names the entry being made) the last of them is the first byte it writes itself: the byte-serial copy
// in ascending order is right for both.
// libtiff keeps counting entries past 4095 and stops with an error when entry 5119 would be made, that is at a data code
// numbered LZW_SEGMENT_CODES behind a Clear (a Clear or EOI of that number is still taken); so does this core.
// Nothing here reads outside the scan or writes outside the tile whatever the bytes are: every code's bits are compared with
// the scan's end before they are fetched, a source range always lies below the write position, and the loop advances by at
// least 9 bits of the scan per turn.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/sequoia_hip.h"

#if defined(__HIPCC__)
#define LZW_HD __host__ __device__ static inline
#else
#define LZW_HD static inline
#endif

#define LZW_CLEAR 256u
#define LZW_EOI 257u
#define LZW_FIRST 258u
#define LZW_TABLE_CODES (4096 - 258)     // codes of a segment a 12-bit code can name: entries 258..4095
#define LZW_SEGMENT_CODES 4862           // data codes of a segment libtiff takes: the next would make entry 5119

struct LzwEntry { uint32_t pos, len; };  // the string of a code of the current segment: where it lies in the output, its bytes

LZW_HD int lzw_code_width(uint32_t j) { return j < 254 ? 9 : j < 766 ? 10 : j < 1790 ? 11 : 12; }

// bits between the end of the Clear and the start of code j
LZW_HD uint64_t lzw_code_bit(uint32_t j) {
    if (j <= 254) return 9ull * j;
    if (j <= 766) return 9ull * 254 + 10ull * (j - 254);
    if (j <= 1790) return 9ull * 254 + 10ull * 512 + 11ull * (j - 766);
    return 9ull * 254 + 10ull * 512 + 11ull * 1024 + 12ull * (j - 1790);
}

// the `width` bits at `bit` of scan[0 .. len): the caller has checked bit + width <= 8 * len
LZW_HD uint32_t lzw_fetch(const uint8_t* scan, uint32_t len, uint64_t bit, int width) {
    const uint64_t b = bit >> 3;
    uint32_t v = (uint32_t)scan[b] << 16;
    if (b + 1 < len) v |= (uint32_t)scan[b + 1] << 8;
    if (b + 2 < len) v |= (uint32_t)scan[b + 2];
    return (v >> (24 - (int)(bit & 7) - width)) & ((1u << width) - 1u);
}

// What a code read as code j of its segment is: SQ_LZW_OK for a literal or a valid entry, else the status it ends the tile with.
LZW_HD int lzw_code_status(uint32_t code, uint32_t j) {
    if (code == LZW_EOI) return SQ_LZW_EARLY_EOI;
    if (j >= LZW_SEGMENT_CODES) return SQ_LZW_TABLE_FULL;
    if (code >= LZW_FIRST && code - LZW_FIRST + 1 > j) return SQ_LZW_BAD_CODE;
    return SQ_LZW_OK;
}

LZW_HD int lzw_range_status(const int32_t* row, unsigned long long scans_bytes) {
    const long long off = row[0], len = row[1];
    if (off < 0 || len < 1 || (unsigned long long)(off + len) > scans_bytes) return SQ_LZW_BAD_RANGE;
    return SQ_LZW_OK;
}

// The first `total` bytes of scan[0 .. len) into out[0 .. total); table: LZW_TABLE_CODES entries of scratch.
LZW_HD int lzw_decode_serial(const uint8_t* scan, uint32_t len, uint8_t* out, uint32_t total, LzwEntry* table) {
    const uint64_t nbits = 8ull * len;
    if (nbits < 9) return SQ_LZW_TRUNCATED;
    if (lzw_fetch(scan, len, 0, 9) != LZW_CLEAR) return SQ_LZW_NO_CLEAR;
    uint64_t seg = 9;                    // where code 0 of the segment starts
    uint32_t j = 0, at = 0;
    while (at < total) {
        const int width = lzw_code_width(j);
        const uint64_t bit = seg + lzw_code_bit(j);
        if (bit + width > nbits) return SQ_LZW_TRUNCATED;
        const uint32_t code = lzw_fetch(scan, len, bit, width);
        if (code == LZW_CLEAR) { seg = bit + width; j = 0; continue; }
        const int rc = lzw_code_status(code, j);
        if (rc != SQ_LZW_OK) return rc;
        uint32_t n = 1;
        if (code < 256) {
            out[at] = (uint8_t)code;
        } else {
            const LzwEntry e = table[code - LZW_FIRST];
            n = e.len + 1;
            const uint32_t m = n < total - at ? n : total - at;
            for (uint32_t k = 0; k < m; k++) out[at + k] = out[e.pos + k];
        }
        if (j < LZW_TABLE_CODES) { table[j].pos = at; table[j].len = n; }
        at += n < total - at ? n : total - at;
        j++;
    }
    return SQ_LZW_OK;
}

// Chunky RGB bytes of one tile -> three planes; predictor 2: the running sum modulo 256 along each row, per channel.
LZW_HD void lzw_planes_serial(const uint8_t* chunky, int tile_w, int tile_h, int predictor, uint8_t* planes) {
    const size_t plane = (size_t)tile_w * tile_h;
    for (int y = 0; y < tile_h; y++) {
        uint8_t acc[3] = {0, 0, 0};
        for (int x = 0; x < tile_w; x++)
            for (int c = 0; c < 3; c++) {
                const uint8_t v = chunky[((size_t)y * tile_w + x) * 3 + c];
                acc[c] = predictor == 2 ? (uint8_t)(acc[c] + v) : v;
                planes[c * plane + (size_t)y * tile_w + x] = acc[c];
            }
    }
}
