// JPEG 2000 decode core shared by the device kernels (j2kdec.hip) and the host check program (tools/j2k_hostcheck.cpp):
// parameter-set check, the layout of precinct-bands and code-blocks, the packet-header parser (bit reader with stuffing, tag
// trees), the MQ decoder and the three coding passes, dequantisation, the inverse 5/3 and 9/7 wavelets and the inverse
// component transforms, as include/sequoia_hip.h ("JPEG 2000 tiles") specifies them.  Nothing here reads outside what it is
// handed: every stream byte is compared with its end (a code-block reads FF past its bytes), every record index with the
// counts of the layout, and no loop's trip count depends on stream content without a bound known before it starts (bits of a
// tag-tree walk <= its threshold, Lblock <= 32, passes <= 3 planes - 2, renormalisation <= 15 shifts, packets = layers x
// resolutions x components x precincts).  Integer sums a damaged stream can drive out of 32 bits are formed in uint32_t.
// The float path must round every product and sum on its own (no contraction): the including file sets the pragma or flag.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include "../../include/sequoia_hip.h"

#if defined(__HIPCC__)
#define J2K_HD __host__ __device__ static inline
#else
#define J2K_HD static inline
#endif
#ifndef J2K_HIT
#define J2K_HIT(cx)                      // the host program counts the MQ contexts the fixtures reach
#endif

#define J2K_MAX_LEVELS 8
#define J2K_BANDS 25
#define J2K_SET_WORDS 52                 // per component: guard, style, 25 x (exponent, mantissa)
#define J2K_FLAG_SIG 1
#define J2K_FLAG_NEG 2
#define J2K_FLAG_VISITED 4
#define J2K_FLAG_REFINED 8
#define J2K_BLOCK_MAX 64
#define J2K_FLAG_BYTES ((J2K_BLOCK_MAX + 2) * (J2K_BLOCK_MAX + 2))

// Qe | next state after MPS << 16 | after LPS << 22 | switch << 28
#define J2K_MQ(qe, nm, nl, sw) ((uint32_t)(qe) | ((uint32_t)(nm) << 16) | ((uint32_t)(nl) << 22) | ((uint32_t)(sw) << 28))
#define J2K_MQ_TABLE_INIT { \
    J2K_MQ(0x5601, 1, 1, 1), J2K_MQ(0x3401, 2, 6, 0), J2K_MQ(0x1801, 3, 9, 0), J2K_MQ(0x0AC1, 4, 12, 0), J2K_MQ(0x0521, 5, 29, 0), \
    J2K_MQ(0x0221, 38, 33, 0), J2K_MQ(0x5601, 7, 6, 1), J2K_MQ(0x5401, 8, 14, 0), J2K_MQ(0x4801, 9, 14, 0), J2K_MQ(0x3801, 10, 14, 0), \
    J2K_MQ(0x3001, 11, 17, 0), J2K_MQ(0x2401, 12, 18, 0), J2K_MQ(0x1C01, 13, 20, 0), J2K_MQ(0x1601, 29, 21, 0), J2K_MQ(0x5601, 15, 14, 1), \
    J2K_MQ(0x5401, 16, 14, 0), J2K_MQ(0x5101, 17, 15, 0), J2K_MQ(0x4801, 18, 16, 0), J2K_MQ(0x3801, 19, 17, 0), J2K_MQ(0x3401, 20, 18, 0), \
    J2K_MQ(0x3001, 21, 19, 0), J2K_MQ(0x2801, 22, 19, 0), J2K_MQ(0x2401, 23, 20, 0), J2K_MQ(0x2201, 24, 21, 0), J2K_MQ(0x1C01, 25, 22, 0), \
    J2K_MQ(0x1801, 26, 23, 0), J2K_MQ(0x1601, 27, 24, 0), J2K_MQ(0x1401, 28, 25, 0), J2K_MQ(0x1201, 29, 26, 0), J2K_MQ(0x1101, 30, 27, 0), \
    J2K_MQ(0x0AC1, 31, 28, 0), J2K_MQ(0x09C1, 32, 29, 0), J2K_MQ(0x08A1, 33, 30, 0), J2K_MQ(0x0521, 34, 31, 0), J2K_MQ(0x0441, 35, 32, 0), \
    J2K_MQ(0x02A1, 36, 33, 0), J2K_MQ(0x0221, 37, 34, 0), J2K_MQ(0x0141, 38, 35, 0), J2K_MQ(0x0111, 39, 36, 0), J2K_MQ(0x0085, 40, 37, 0), \
    J2K_MQ(0x0049, 41, 38, 0), J2K_MQ(0x0025, 42, 39, 0), J2K_MQ(0x0015, 43, 40, 0), J2K_MQ(0x0009, 44, 41, 0), J2K_MQ(0x0005, 45, 42, 0), \
    J2K_MQ(0x0001, 45, 43, 0), J2K_MQ(0x5601, 46, 46, 0)}
#define J2K_MQ_STATES 47
#define J2K_CONTEXTS 19

struct J2kParams {
    int tile_w, tile_h, dx;
    int levels, reversible, mct, layers, order, xcb, ycb;
    int ppx[J2K_MAX_LEVELS + 1], ppy[J2K_MAX_LEVELS + 1];
    int guard[3], style[3];
    uint8_t expn[3][J2K_BANDS];
    uint16_t mant[3][J2K_BANDS];
};

struct J2kCounts { int blocks, nodes, bands; };

struct J2kBand {                         // one band of one precinct: its code-block grid and its two tag trees
    int32_t first_block, first_node;
    int16_t nw, nh;
};

struct J2kBlock {
    uint16_t x, y;                       // in the component's coefficient plane
    uint8_t w, h, comp, orient;          // orient: 0 LL, 1 HL, 2 LH, 3 HH
    uint8_t planes, zero_planes, lblock, included;
    uint16_t passes, pad;
    uint32_t off, len, cur, seg;         // bytes: where, how many, gather cursor, the current packet's contribution
    float step;                          // irreversible: the band's step
};

struct J2kNode { uint8_t low, value; };  // value 255: not known yet

struct J2kTile {                         // what the later stages read of a tile
    int32_t status, n_blocks, gathered, levels, reversible, mct, dx, pad;
    int32_t band_first[3][J2K_MAX_LEVELS + 1];
};

J2K_HD int j2k_ceil_div(int a, int b) { return (a + b - 1) / b; }
J2K_HD int j2k_comp_w(const J2kParams* P, int c) { return c == 0 ? P->tile_w : j2k_ceil_div(P->tile_w, P->dx); }
J2K_HD int j2k_res_extent(int full, int levels, int r) { return j2k_ceil_div(full, 1 << (levels - r)); }
J2K_HD int32_t j2k_word(const uint8_t* p, int i) {
    return (int32_t)((uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24));
}
J2K_HD float j2k_as_float(int32_t v) { float f; memcpy(&f, &v, 4); return f; }
J2K_HD int32_t j2k_as_int(float f) { int32_t v; memcpy(&v, &f, 4); return v; }
J2K_HD int32_t j2k_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
J2K_HD int32_t j2k_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

J2K_HD int j2k_precincts(const J2kParams* P, int c, int r, int* across) {
    const int rw = j2k_res_extent(j2k_comp_w(P, c), P->levels, r), rh = j2k_res_extent(P->tile_h, P->levels, r);
    const int nx = (int)(((long long)rw + (1ll << P->ppx[r]) - 1) >> P->ppx[r]), ny = (int)(((long long)rh + (1ll << P->ppy[r]) - 1) >> P->ppy[r]);
    if (across) *across = nx;
    return nx * ny;
}

// The block of SQ_J2K_PARAM_BYTES -> P; false for any field outside include/sequoia_hip.h's ranges.
J2K_HD bool j2k_params_load(const uint8_t* set, int tile_w, int tile_h, J2kParams* P) {
    if (tile_w < 16 || tile_w > SQ_JPEG_MAX_TILE || tile_h < 16 || tile_h > SQ_JPEG_MAX_TILE || (tile_w & 15) || (tile_h & 15)) return false;
    if (j2k_word(set, 0) != SQ_J2K_PARAM_MAGIC) return false;
    P->tile_w = tile_w; P->tile_h = tile_h;
    P->dx = j2k_word(set, 1); P->levels = j2k_word(set, 2); P->reversible = j2k_word(set, 3); P->mct = j2k_word(set, 4);
    P->layers = j2k_word(set, 5); P->order = j2k_word(set, 6); P->xcb = j2k_word(set, 7); P->ycb = j2k_word(set, 8);
    if (P->dx < 1 || P->dx > 2 || P->levels < 0 || P->levels > J2K_MAX_LEVELS || (P->reversible & ~1) || (P->mct & ~1) || (P->mct && P->dx != 1))
        return false;
    if (P->layers < 1 || P->layers > 32 || P->order < 0 || P->order > 4 || P->xcb < 2 || P->xcb > 6 || P->ycb < 2 || P->ycb > 6) return false;
    for (int r = 0; r <= J2K_MAX_LEVELS; r++) {
        const int v = j2k_word(set, 9 + r);
        P->ppx[r] = v & 15; P->ppy[r] = (v >> 4) & 15;
        if (v < 0 || v > 255 || (r > 0 && r <= P->levels && (P->ppx[r] < 1 || P->ppy[r] < 1))) return false;
    }
    for (int c = 0; c < 3; c++) {
        const int at = 18 + c * J2K_SET_WORDS;
        P->guard[c] = j2k_word(set, at); P->style[c] = j2k_word(set, at + 1);
        if (P->guard[c] < 0 || P->guard[c] > 7 || P->style[c] < 0 || P->style[c] > 2 || (P->reversible && P->style[c] != 0) ||
            (!P->reversible && P->style[c] == 0)) return false;
        for (int b = 0; b < J2K_BANDS; b++) {
            const int e = j2k_word(set, at + 2 + 2 * b), m = j2k_word(set, at + 3 + 2 * b);
            if (e < 0 || e > 31 || m < 0 || m > 2047) return false;
            if (b < 3 * P->levels + 1 && (P->guard[c] + e - 1 < 0 || P->guard[c] + e - 1 > SQ_J2K_MAX_PLANES)) return false;
            P->expn[c][b] = (uint8_t)e; P->mant[c][b] = (uint16_t)m;
        }
        for (int r = 0; r <= P->levels; r++) {
            const int n = j2k_precincts(P, c, r, nullptr);
            if (n > SQ_J2K_MAX_PRECINCTS || (P->order >= 2 && n != 1)) return false;
        }
    }
    return true;
}

J2K_HD int j2k_tree_nodes(int w, int h) {
    if (w < 1 || h < 1) return 0;
    int n = 0;
    for (int l = 0; l < 16; l++) {
        n += w * h;
        if (w <= 1 && h <= 1) break;
        w = (w + 1) >> 1; h = (h + 1) >> 1;
    }
    return n;
}

// Extent and plane position of band `orient` of resolution r of component c.
J2K_HD void j2k_band_geom(const J2kParams* P, int c, int r, int orient, int* x0, int* y0, int* w, int* h) {
    const int cw = j2k_comp_w(P, c), ch = P->tile_h;
    const int rw = j2k_res_extent(cw, P->levels, r), rh = j2k_res_extent(ch, P->levels, r);
    if (r == 0) { *x0 = 0; *y0 = 0; *w = rw; *h = rh; return; }
    const int lw = (rw + 1) >> 1, lh = (rh + 1) >> 1;
    *x0 = (orient & 1) ? lw : 0; *y0 = (orient & 2) ? lh : 0;
    *w = (orient & 1) ? rw - lw : lw; *h = (orient & 2) ? rh - lh : lh;
}

// Counts of a parameter set; with records, fills them (and T->band_first) as long as they fit `cap`.  False: they do not fit.
J2K_HD bool j2k_layout(const J2kParams* P, J2kCounts* n, J2kTile* T, J2kBand* bands, J2kBlock* blocks, J2kNode* nodes, const J2kCounts* cap) {
    n->blocks = n->nodes = n->bands = 0;
    for (int c = 0; c < 3; c++)
        for (int r = 0; r <= P->levels; r++) {
            if (T) T->band_first[c][r] = n->bands;
            int across = 1;
            const int np = j2k_precincts(P, c, r, &across);
            const int px_exp = r ? P->ppx[r] - 1 : P->ppx[r], py_exp = r ? P->ppy[r] - 1 : P->ppy[r];
            const int xcb = P->xcb < px_exp ? P->xcb : px_exp, ycb = P->ycb < py_exp ? P->ycb : py_exp;
            for (int p = 0; p < np; p++)
                for (int o = (r ? 1 : 0); o <= (r ? 3 : 0); o++) {
                    int bx, by, bw, bh;
                    j2k_band_geom(P, c, r, o, &bx, &by, &bw, &bh);
                    const long long qx0 = (long long)(p % across) << px_exp, qy0 = (long long)(p / across) << py_exp;
                    long long qx1 = qx0 + (1ll << px_exp), qy1 = qy0 + (1ll << py_exp);
                    if (qx1 > bw) qx1 = bw;
                    if (qy1 > bh) qy1 = bh;
                    const int nw = qx1 > qx0 ? (int)((qx1 - qx0 + (1 << xcb) - 1) >> xcb) : 0;
                    const int nh = qy1 > qy0 ? (int)((qy1 - qy0 + (1 << ycb) - 1) >> ycb) : 0;
                    const int cells = (nw && nh) ? nw * nh : 0, tree = j2k_tree_nodes(cells ? nw : 0, nh);
                    if (bands) {
                        if (n->bands + 1 > cap->bands || n->blocks + cells > cap->blocks || n->nodes + 2 * tree > cap->nodes) return false;
                        J2kBand* B = bands + n->bands;
                        B->first_block = n->blocks; B->first_node = n->nodes; B->nw = (int16_t)(cells ? nw : 0); B->nh = (int16_t)(cells ? nh : 0);
                        const int sb = r ? 3 * (r - 1) + o : 0, e = P->expn[c][sb];
                        const int gain = o == 0 ? 0 : (o == 3 ? 2 : 1);
                        const float step = (1.0f + (float)P->mant[c][sb] * (1.0f / 2048.0f)) * ldexpf(1.0f, 8 + gain - e);
                        for (int i = 0; i < cells; i++) {
                            J2kBlock* K = blocks + n->blocks + i;
                            const int x = (int)qx0 + ((i % nw) << xcb), y = (int)qy0 + ((i / nw) << ycb);
                            const int x1 = x + (1 << xcb) < (int)qx1 ? x + (1 << xcb) : (int)qx1, y1 = y + (1 << ycb) < (int)qy1 ? y + (1 << ycb) : (int)qy1;
                            K->x = (uint16_t)(bx + x); K->y = (uint16_t)(by + y); K->w = (uint8_t)(x1 - x); K->h = (uint8_t)(y1 - y);
                            K->comp = (uint8_t)c; K->orient = (uint8_t)o; K->planes = (uint8_t)(P->guard[c] + e - 1);
                            K->zero_planes = 0; K->lblock = 3; K->included = 0; K->passes = 0; K->pad = 0;
                            K->off = K->len = K->cur = K->seg = 0; K->step = step;
                        }
                        for (int i = 0; i < 2 * tree; i++) { nodes[n->nodes + i].low = 0; nodes[n->nodes + i].value = 255; }
                    }
                    n->bands += 1; n->blocks += cells; n->nodes += 2 * tree;
                }
        }
    return true;
}

// ---- packet headers -----------------------------------------------------------------------------------------------
struct J2kBits { const uint8_t* d; uint32_t pos, end, acc; int n, after_ff, err; };

J2K_HD int j2k_bit(J2kBits* b) {
    if (b->n == 0) {
        if (b->pos >= b->end) { b->err = 1; return 0; }
        b->acc = b->d[b->pos++];
        b->n = b->after_ff ? 7 : 8;
        b->after_ff = b->acc == 0xFF;
    }
    b->n--;
    return (int)((b->acc >> b->n) & 1);
}
J2K_HD uint32_t j2k_bits(J2kBits* b, int count) {          // count <= 32
    uint32_t v = 0;
    for (int i = 0; i < count; i++) v = (v << 1) | (uint32_t)j2k_bit(b);
    return v;
}
J2K_HD void j2k_align(J2kBits* b) {
    b->n = 0;
    if (b->after_ff) {
        if (b->pos >= b->end) b->err = 1; else b->pos++;
        b->after_ff = 0;
    }
}

// One tag-tree query: is the leaf's value below `threshold` (<= 64)?  Reads at most `threshold` bits per level.
J2K_HD bool j2k_tag(J2kNode* tree, int nw, int nh, int x, int y, int threshold, J2kBits* b) {
    int top = 0;
    for (int w = nw, h = nh; top < 15 && (w > 1 || h > 1); top++) { w = (w + 1) >> 1; h = (h + 1) >> 1; }
    int low = 0, value = 255;
    for (int l = top; l >= 0; l--) {
        int off = 0, w = nw, h = nh;
        for (int i = 0; i < l; i++) { off += w * h; w = (w + 1) >> 1; h = (h + 1) >> 1; }
        J2kNode* nd = tree + off + (y >> l) * w + (x >> l);
        if (low > nd->low) nd->low = (uint8_t)low; else low = nd->low;
        value = nd->value;
        for (int i = 0; i < threshold && low < threshold && low < value; i++) {
            if (j2k_bit(b)) { value = low; nd->value = (uint8_t)low; } else low++;
        }
        nd->low = (uint8_t)low;
    }
    return value < threshold;
}

J2K_HD int j2k_log2(uint32_t v) { int n = 0; for (int i = 0; i < 31 && (v >> 1); i++) { v >>= 1; n++; } return n; }

// One walk over the packets of a tile.  phase 0: headers checked, lengths summed (one layer: the bytes stay where they are,
// off = their place in the stream buffer); phase 1 (several layers): the contributions copied behind one another at `gather`.
J2K_HD int j2k_walk(const J2kParams* P, const uint8_t* s, uint32_t base, uint32_t len, const J2kTile* T, const J2kBand* bands,
                    J2kBlock* blocks, J2kNode* nodes, uint8_t* gather, int phase) {
    uint32_t pos = base;
    const uint32_t end = base + len;
    const int R = P->levels + 1, L = P->layers;
    int ext[3];
    ext[0] = P->order == 0 ? L : (P->order <= 2 ? R : (P->order == 3 ? 1 : 3));
    ext[1] = P->order == 0 ? R : (P->order == 1 ? L : (P->order == 2 ? 1 : (P->order == 3 ? 3 : 1)));
    ext[2] = P->order <= 1 ? 3 : (P->order == 2 ? 3 : R);
    for (int i0 = 0; i0 < ext[0]; i0++)
        for (int i1 = 0; i1 < ext[1]; i1++)
            for (int i2 = 0; i2 < ext[2]; i2++) {
                int l, r, c;                                             // orders 2..4: one precinct, the layer innermost
                if (P->order == 0) { l = i0; r = i1; c = i2; }
                else if (P->order == 1) { r = i0; l = i1; c = i2; }
                else if (P->order == 2) { r = i0; c = i2; l = -1; }
                else if (P->order == 3) { c = i1; r = i2; l = -1; }
                else { c = i0; r = i2; l = -1; }
                const int inner = l < 0 ? L : j2k_precincts(P, c, r, nullptr);
                for (int i3 = 0; i3 < inner; i3++) {
                    const int layer = l < 0 ? i3 : l, p = l < 0 ? 0 : i3;
                    const int nb = r ? 3 : 1;
                    const J2kBand* B0 = bands + T->band_first[c][r] + p * nb;
                    J2kBits b;
                    b.d = s; b.pos = pos; b.end = end; b.acc = 0; b.n = 0; b.after_ff = 0; b.err = 0;
                    const int present = j2k_bit(&b);
                    if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                    if (present)
                        for (int o = 0; o < nb; o++) {
                            const J2kBand* B = B0 + o;
                            const int tree = j2k_tree_nodes(B->nw, B->nh);
                            for (int i = 0; i < B->nw * B->nh; i++) {
                                J2kBlock* K = blocks + B->first_block + i;
                                const int cx = i % B->nw, cy = i / B->nw;
                                K->seg = 0;
                                const bool in = K->included ? j2k_bit(&b) != 0 : j2k_tag(nodes + B->first_node, B->nw, B->nh, cx, cy, layer + 1, &b);
                                if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                                if (!in) continue;
                                if (!K->included) {
                                    int z = 1;
                                    while (z <= SQ_J2K_MAX_PLANES + 2 && !j2k_tag(nodes + B->first_node + tree, B->nw, B->nh, cx, cy, z, &b) && !b.err) z++;
                                    if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                                    if (z - 1 > K->planes) return SQ_J2K_BAD_LENGTH;
                                    K->zero_planes = (uint8_t)(z - 1); K->included = 1; K->lblock = 3;
                                }
                                int np = 1;
                                if (j2k_bit(&b)) {
                                    np = 2;
                                    if (j2k_bit(&b)) {
                                        np = 3 + (int)j2k_bits(&b, 2);
                                        if (np == 6) {
                                            np = 6 + (int)j2k_bits(&b, 5);
                                            if (np == 37) np = 37 + (int)j2k_bits(&b, 7);
                                        }
                                    }
                                }
                                int lblock = K->lblock;
                                while (lblock <= 32 && j2k_bit(&b)) lblock++;
                                if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                                const int nbits = lblock + j2k_log2((uint32_t)np);
                                if (nbits > 32) return SQ_J2K_BAD_LENGTH;
                                const uint32_t seg = j2k_bits(&b, nbits);
                                if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                                if (K->passes + np > 3 * (K->planes - K->zero_planes) - 2 || seg > len) return SQ_J2K_BAD_LENGTH;
                                K->lblock = (uint8_t)lblock; K->passes = (uint16_t)(K->passes + np); K->seg = seg;
                            }
                        }
                    j2k_align(&b);
                    if (b.err) return SQ_J2K_TRUNCATED_HEADER;
                    pos = b.pos;
                    if (!present) continue;
                    for (int o = 0; o < nb; o++) {
                        const J2kBand* B = B0 + o;
                        for (int i = 0; i < B->nw * B->nh; i++) {
                            J2kBlock* K = blocks + B->first_block + i;
                            const uint32_t seg = K->seg;
                            if (!seg) continue;
                            K->seg = 0;
                            if (seg > end - pos) return SQ_J2K_TRUNCATED_BODY;
                            if (phase == 0) {
                                if (L == 1) K->off = pos;
                                K->len += seg;
                            } else {
                                for (uint32_t j = 0; j < seg; j++) gather[K->off + K->cur + j] = s[pos + j];
                                K->cur += seg;
                            }
                            pos += seg;
                        }
                    }
                }
            }
    return SQ_J2K_OK;
}

// Everything before the code-blocks for one tile: parameter check, layout, the packet walk(s).  `gather`: `streams_bytes`
// bytes, of which the tile writes its own range [base, base + len).  Returns the status; T, bands, blocks, nodes are the tile's.
J2K_HD int j2k_tile_packets(const uint8_t* set_bytes, int n_sets, const int32_t* row, const uint8_t* streams, unsigned long long streams_bytes,
                            int tile_w, int tile_h, const J2kCounts* cap, J2kTile* T, J2kBand* bands, J2kBlock* blocks, J2kNode* nodes,
                            uint8_t* gather) {
    T->status = SQ_J2K_OK; T->n_blocks = 0; T->gathered = 0; T->levels = 0; T->reversible = 1; T->mct = 0; T->dx = 1; T->pad = 0;
    if (row[2] < 0 || row[2] >= n_sets) return SQ_J2K_BAD_PARAM;
    J2kParams P;
    if (!j2k_params_load(set_bytes + (size_t)row[2] * SQ_J2K_PARAM_BYTES, tile_w, tile_h, &P)) return SQ_J2K_BAD_PARAM;
    if (row[0] < 0 || row[1] < 1 || (unsigned long long)row[0] + (unsigned long long)row[1] > streams_bytes) return SQ_J2K_BAD_RANGE;
    J2kCounts n;
    if (!j2k_layout(&P, &n, T, bands, blocks, nodes, cap)) return SQ_J2K_BAD_PARAM;
    T->levels = P.levels; T->reversible = P.reversible; T->mct = P.mct; T->dx = P.dx;
    const uint32_t base = (uint32_t)row[0], len = (uint32_t)row[1];
    int rc = j2k_walk(&P, streams, base, len, T, bands, blocks, nodes, gather, 0);
    if (rc != SQ_J2K_OK) return rc;
    if (P.layers > 1) {
        uint32_t at = base;
        for (int i = 0; i < n.blocks; i++) {
            J2kBlock* K = blocks + i;
            K->off = at; at += K->len;                                  // the sum is at most len: every segment was inside the stream
            K->included = 0; K->lblock = 3; K->passes = 0; K->cur = 0; K->seg = 0;
        }
        for (int i = 0; i < n.nodes; i++) { nodes[i].low = 0; nodes[i].value = 255; }
        rc = j2k_walk(&P, streams, base, len, T, bands, blocks, nodes, gather, 1);
        if (rc != SQ_J2K_OK) return rc;
        T->gathered = 1;
    }
    T->n_blocks = n.blocks;
    return SQ_J2K_OK;
}

// ---- code-blocks ----------------------------------------------------------------------------------------------------
struct J2kMq { const uint8_t* d; uint32_t pos, len, a, c; int ct; uint8_t* cx; const uint32_t* table; };

J2K_HD uint32_t j2k_mq_byte(const J2kMq* m, uint32_t i) { return i < m->len ? m->d[i] : 0xFFu; }
J2K_HD void j2k_mq_bytein(J2kMq* m) {
    if (j2k_mq_byte(m, m->pos) == 0xFF) {
        const uint32_t next = j2k_mq_byte(m, m->pos + 1);
        if (next > 0x8F) { m->c += 0xFF00; m->ct = 8; }
        else { m->pos++; m->c += next << 9; m->ct = 7; }
    } else {
        m->pos++;
        m->c += j2k_mq_byte(m, m->pos) << 8;
        m->ct = 8;
    }
}
J2K_HD void j2k_mq_init(J2kMq* m, const uint8_t* d, uint32_t len, uint8_t* cx, const uint32_t* table) {
    m->d = d; m->len = len; m->pos = 0; m->cx = cx; m->table = table;
    for (int i = 0; i < J2K_CONTEXTS; i++) cx[i] = 0;
    cx[0] = 4 << 1; cx[17] = 3 << 1; cx[18] = 46 << 1;                  // state << 1 | most probable symbol
    m->c = j2k_mq_byte(m, 0) << 16;
    j2k_mq_bytein(m);
    m->c <<= 7; m->ct -= 7; m->a = 0x8000;
}
J2K_HD int j2k_mq_decode(J2kMq* m, int cx) {
    J2K_HIT(cx);
    const uint32_t st = m->cx[cx], e = m->table[st >> 1], qe = e & 0xFFFF;
    int mps = (int)(st & 1), d;
    bool lps;
    m->a -= qe;
    if ((m->c >> 16) < qe) {
        lps = !(m->a < qe);
        m->a = qe;
    } else {
        m->c -= qe << 16;
        if (m->a & 0x8000) return mps;
        lps = m->a < qe;
    }
    if (lps) {
        d = 1 - mps;
        if ((e >> 28) & 1) mps = 1 - mps;
        m->cx[cx] = (uint8_t)((((e >> 22) & 63) << 1) | (uint32_t)mps);
    } else {
        d = mps;
        m->cx[cx] = (uint8_t)((((e >> 16) & 63) << 1) | (uint32_t)mps);
    }
    for (int i = 0; i < 16; i++) {
        if (m->ct == 0) j2k_mq_bytein(m);
        m->a <<= 1; m->c <<= 1; m->ct--;
        if (m->a & 0x8000) break;
    }
    return d;
}

J2K_HD int j2k_zc_context(const uint8_t* f, int fs, int orient) {
    int h = (f[-1] & 1) + (f[1] & 1), v = (f[-fs] & 1) + (f[fs] & 1);
    const int d = (f[-fs - 1] & 1) + (f[-fs + 1] & 1) + (f[fs - 1] & 1) + (f[fs + 1] & 1);
    if (orient == 3) {
        const int hv = h + v;
        if (d >= 3) return 8;
        if (d == 2) return hv >= 1 ? 7 : 6;
        if (d == 1) return hv >= 2 ? 5 : (hv == 1 ? 4 : 3);
        return hv >= 2 ? 2 : hv;
    }
    if (orient == 1) { const int t = h; h = v; v = t; }
    if (h == 2) return 8;
    if (h == 1) return v >= 1 ? 7 : (d >= 1 ? 6 : 5);
    if (v == 2) return 4;
    if (v == 1) return 3;
    return d >= 2 ? 2 : d;
}
J2K_HD int j2k_sign_part(uint8_t a, uint8_t b) {
    int s = ((a & 1) ? ((a & J2K_FLAG_NEG) ? -1 : 1) : 0) + ((b & 1) ? ((b & J2K_FLAG_NEG) ? -1 : 1) : 0);
    return s > 1 ? 1 : (s < -1 ? -1 : s);
}
J2K_HD int j2k_decode_sign(J2kMq* m, const uint8_t* f, int fs) {
    const int h = j2k_sign_part(f[-1], f[1]), v = j2k_sign_part(f[-fs], f[fs]);
    int cx, flip = 0;
    if (h == 1) cx = v == 1 ? 13 : (v == 0 ? 12 : 11);
    else if (h == 0) { cx = v == 0 ? 9 : 10; flip = v == -1; }
    else { cx = v == 1 ? 11 : (v == 0 ? 12 : 13); flip = 1; }
    return j2k_mq_decode(m, cx) ^ flip;
}
J2K_HD void j2k_become_significant(J2kMq* m, uint8_t* f, int fs, uint32_t* v, int plane) {
    const int neg = j2k_decode_sign(m, f, fs);
    *f |= (uint8_t)(J2K_FLAG_SIG | (neg ? J2K_FLAG_NEG : 0));
    *v = (3u << plane) | (neg ? 0x80000000u : 0u);
}

// One code-block: `coef` (w x h, zero) receives doubled magnitudes with the sign in bit 31; `flags` ((w + 2) x (h + 2), zero)
// and `cx` (J2K_CONTEXTS bytes) are working storage.
J2K_HD void j2k_block_decode(const J2kBlock* K, const uint8_t* data, uint32_t* coef, uint8_t* flags, uint8_t* cx, const uint32_t* table) {
    const int w = K->w, h = K->h, fs = w + 2, orient = K->orient;
    const int planes = K->planes - K->zero_planes;
    if (!K->included || K->passes == 0 || planes < 1 || (int)K->passes > 3 * planes - 2) return;
    J2kMq m;
    j2k_mq_init(&m, data, K->len, cx, table);
    int plane = planes - 1, type = 2;
    for (int pass = 0; pass < (int)K->passes; pass++) {
        for (int y0 = 0; y0 < h; y0 += 4) {
            const int rows = h - y0 < 4 ? h - y0 : 4;
            for (int x = 0; x < w; x++) {
                uint8_t* f = flags + (y0 + 1) * fs + x + 1;
                uint32_t* v = coef + y0 * w + x;
                int first = 0;
                if (type == 2 && rows == 4) {
                    bool quiet = true;
                    for (int j = 0; j < 4; j++) quiet = quiet && f[j * fs] == 0 && j2k_zc_context(f + j * fs, fs, orient) == 0;
                    if (quiet) {
                        if (!j2k_mq_decode(&m, 17)) continue;
                        first = j2k_mq_decode(&m, 18) << 1;
                        first |= j2k_mq_decode(&m, 18);
                        j2k_become_significant(&m, f + first * fs, fs, v + first * w, plane);
                        first++;
                    }
                }
                for (int j = first; j < rows; j++) {
                    uint8_t* fj = f + j * fs;
                    uint32_t* vj = v + j * w;
                    if (type == 0) {
                        if (*fj & J2K_FLAG_SIG) continue;
                        const int z = j2k_zc_context(fj, fs, orient);
                        if (z == 0) continue;
                        if (j2k_mq_decode(&m, z)) j2k_become_significant(&m, fj, fs, vj, plane);
                        *fj |= J2K_FLAG_VISITED;
                    } else if (type == 1) {
                        if ((*fj & (J2K_FLAG_SIG | J2K_FLAG_VISITED)) != J2K_FLAG_SIG) continue;
                        const int r = (*fj & J2K_FLAG_REFINED) ? 16 : (j2k_zc_context(fj, fs, 0) ? 15 : 14);
                        const uint32_t half = 1u << plane;
                        *vj = j2k_mq_decode(&m, r) ? *vj + half : *vj - half;
                        *fj |= J2K_FLAG_REFINED;
                    } else {
                        if (*fj & (J2K_FLAG_SIG | J2K_FLAG_VISITED)) continue;
                        if (j2k_mq_decode(&m, j2k_zc_context(fj, fs, orient))) j2k_become_significant(&m, fj, fs, vj, plane);
                    }
                }
            }
        }
        if (type == 2) {
            for (int i = 0; i < (h + 2) * fs; i++) flags[i] &= (uint8_t)~J2K_FLAG_VISITED;
            type = 0; plane--;
        } else type++;
    }
}

// A decoded sample as the wavelet takes it: int32, or float bits on the irreversible path.
J2K_HD int32_t j2k_dequant(uint32_t v, int reversible, float step) {
    const uint32_t mag = v & 0x7FFFFFFFu;
    if (reversible) { const int32_t q = (int32_t)(mag >> 1); return (v >> 31) ? -q : q; }
    const float f = ((float)mag * 0.5f) * step;
    return j2k_as_int((v >> 31) ? -f : f);
}

// ---- inverse wavelet ------------------------------------------------------------------------------------------------
#define J2K_K 1.230174105f
#define J2K_INV_K (1.0f / 1.230174105f)
J2K_HD int j2k_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// Interleave one sample of a line of n (low half first, `lo` low samples) into position i, with the 9/7 scaling.
J2K_HD int32_t j2k_interleaved(int32_t v, int odd, int reversible) {
    if (reversible) return v;
    return j2k_as_int(j2k_as_float(v) * (odd ? J2K_INV_K : J2K_K));
}
// Lifting step `step` on sample i of a line of n >= 2 whose neighbours are a and b: 5/3 has steps 0 (even) and 1 (odd), 9/7
// steps 0..3 (even, odd, even, odd).
J2K_HD int32_t j2k_lift(int32_t x, int32_t a, int32_t b, int step, int reversible) {
    if (reversible) {
        const int32_t s = j2k_add(a, b);
        return step == 0 ? j2k_sub(x, j2k_add(s, 2) >> 2) : j2k_add(x, s >> 1);
    }
    const float k = step == 0 ? 0.443506852f : (step == 1 ? 0.882911075f : (step == 2 ? -0.052980118f : -1.586134342f));
    const float sum = j2k_as_float(a) + j2k_as_float(b);
    const float prod = k * sum;
    return j2k_as_int(j2k_as_float(x) - prod);
}

// The inverse wavelet of one component in place in `a` (stride S), `t` a second plane; thread `tid` of `nt`, `sync` between steps.
template <class Sync>
J2K_HD void j2k_idwt(int comp_w, int comp_h, int levels, int reversible, int32_t* a, int32_t* t, int S, int tid, int nt, Sync sync) {
    const int steps = reversible ? 2 : 4;
    for (int r = 1; r <= levels; r++) {
        const int rw = j2k_res_extent(comp_w, levels, r), rh = j2k_res_extent(comp_h, levels, r);
        const int lw = (rw + 1) >> 1, lh = (rh + 1) >> 1, total = rw * rh;
        for (int i = tid; i < total; i += nt) {
            const int y = i / rw, x = i % rw;
            t[y * S + x] = rw > 1 ? j2k_interleaved(a[y * S + ((x & 1) ? lw + (x >> 1) : (x >> 1))], x & 1, reversible) : a[y * S + x];
        }
        sync();
        if (rw > 1)
            for (int s = 0; s < steps; s++) {
                for (int i = tid; i < total; i += nt) {
                    const int y = i / rw, x = i % rw;
                    if ((x & 1) == (s & 1)) t[y * S + x] = j2k_lift(t[y * S + x], t[y * S + j2k_mirror(x - 1, rw)], t[y * S + j2k_mirror(x + 1, rw)], s, reversible);
                }
                sync();
            }
        for (int i = tid; i < total; i += nt) {
            const int y = i / rw, x = i % rw;
            a[y * S + x] = rh > 1 ? j2k_interleaved(t[((y & 1) ? lh + (y >> 1) : (y >> 1)) * S + x], y & 1, reversible) : t[y * S + x];
        }
        sync();
        if (rh > 1)
            for (int s = 0; s < steps; s++) {
                for (int i = tid; i < total; i += nt) {
                    const int y = i / rw, x = i % rw;
                    if ((y & 1) == (s & 1)) a[y * S + x] = j2k_lift(a[y * S + x], a[j2k_mirror(y - 1, rh) * S + x], a[j2k_mirror(y + 1, rh) * S + x], s, reversible);
                }
                sync();
            }
    }
}

// ---- components -> bytes ----------------------------------------------------------------------------------------------
J2K_HD uint8_t j2k_clamp_int(int32_t v) { v = j2k_add(v, 128); return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
J2K_HD uint8_t j2k_clamp_float(float f) {
    f = rintf(f);
    if (!(f > -1000.0f)) f = -1000.0f;
    if (f > 1000.0f) f = 1000.0f;
    return j2k_clamp_int((int32_t)f);
}
// The three samples of one pixel (wavelet output) -> the three plane bytes.
J2K_HD void j2k_pixel(int32_t c0, int32_t c1, int32_t c2, int reversible, int mct, uint8_t* out) {
    if (reversible) {
        if (mct) {
            const int32_t g = j2k_sub(c0, j2k_add(c1, c2) >> 2);
            const int32_t r = j2k_add(c2, g), b = j2k_add(c1, g);
            c0 = r; c1 = g; c2 = b;
        }
        out[0] = j2k_clamp_int(c0); out[1] = j2k_clamp_int(c1); out[2] = j2k_clamp_int(c2);
        return;
    }
    float y = j2k_as_float(c0), cb = j2k_as_float(c1), cr = j2k_as_float(c2);
    if (mct) {
        const float pr = 1.402f * cr, pg1 = 0.34413f * cb, pg2 = 0.71414f * cr, pb = 1.772f * cb;
        const float r = y + pr, g1 = y - pg1, b = y + pb;
        const float g = g1 - pg2;
        y = r; cb = g; cr = b;
    }
    out[0] = j2k_clamp_float(y); out[1] = j2k_clamp_float(cb); out[2] = j2k_clamp_float(cr);
}
