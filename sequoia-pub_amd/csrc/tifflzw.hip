// LZW and uncompressed tiles of a generic tiled TIFF level -> the planes sq_jpeg_compose_regions reads (include/sequoia_hip.h,
// "LZW and uncompressed tiles").  Three kernels: the wave decoder (one wave and one workgroup per tile: the bit position of a
// code follows from its number behind the last Clear, so the 64 lanes fetch 64 codes at once; an entry is a range of the
// output already written, so the table in LDS is (position, length) and the strings are copied by all lanes), the lane
// decoder (one lane per tile runs lzw_core.h's serial decoder: the in-library reference, and the range check of uncompressed
// tiles) and the plane writer (a wave per row: the running sum of Predictor 2 as a wave scan, chunky bytes to three planes).
// The chunky bytes of a tile go through the workspace in global memory: a 1024 x 1024 tile is 3 MB.  The wave decoder's
// stores are read back by other lanes of the same wave: every such hand-over crosses a __syncthreads() of the one-wave
// workgroup, which orders them at workgroup scope.
#include "sq_common.h"
#include "lzw_core.h"
#include <stdio.h>

namespace {

constexpr int WAVE = 64;
constexpr int LANE_MAX_WAVES = 4096;
constexpr int PLN_THREADS = 256;
constexpr uint32_t R_LITERAL = 1u << 31, R_LATE = 1u << 30, R_POS = (1u << 30) - 1;

struct LzwArgs {
    const uint8_t* scans; unsigned long long scans_bytes;
    const int32_t* tile_table; int n_tiles;
    int lanes;                           // tiles per wave of the lane kernel
    int tile_w, tile_h, compression, predictor;
    uint8_t* chunky;                     // [n_tiles][tile_h][tile_w][3]
    LzwEntry* tables;                    // lane mode: [n_tiles][LZW_TABLE_CODES]
    uint8_t* planes; int32_t* status;
};

__global__ __launch_bounds__(WAVE) void lzw_lane_kernel(LzwArgs a) {
    const int tile = blockIdx.x * a.lanes + threadIdx.x;
    if ((int)threadIdx.x >= a.lanes || tile >= a.n_tiles) return;
    const int32_t* row = a.tile_table + (size_t)tile * SQ_LZW_TILE_WORDS;
    const uint32_t total = 3u * a.tile_w * a.tile_h;
    int rc = lzw_range_status(row, a.scans_bytes);
    if (rc == SQ_LZW_OK) {
        if (a.compression == 1) rc = (uint32_t)row[1] < total ? SQ_LZW_TRUNCATED : SQ_LZW_OK;
        else rc = lzw_decode_serial(a.scans + row[0], (uint32_t)row[1], a.chunky + (size_t)tile * total, total,
                                    a.tables + (size_t)tile * LZW_TABLE_CODES);
    }
    a.status[tile] = rc;
}

// The `width` bits at bit `bit` of the tile's scan, which starts at byte `off` of scans: two aligned dwords of `scans`
// (scans_bytes is a multiple of 16 and the base 16-byte aligned, so a dword inside the buffer is whole).  Bits behind the
// tile's own bytes may come along: the caller has checked bit + width against the scan's end.
__device__ __forceinline__ uint32_t fetch_code(const uint32_t* words, unsigned long long n_words, unsigned long long off, uint64_t bit, int width) {
    const unsigned long long byte = off + (bit >> 3), w = byte >> 2;
    const uint32_t hi = __builtin_bswap32(words[w]);
    const uint32_t lo = w + 1 < n_words ? __builtin_bswap32(words[w + 1]) : 0u;
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    const int o = (int)(byte & 3) * 8 + (int)(bit & 7);
    return (uint32_t)(v >> (64 - o - width)) & ((1u << width) - 1u);
}

__global__ __launch_bounds__(WAVE) void lzw_wave_kernel(LzwArgs a) {
    __shared__ uint32_t t_pos[LZW_TABLE_CODES];
    __shared__ uint16_t t_len[LZW_TABLE_CODES];
    __shared__ uint32_t r_pos[WAVE + 1];                 // where the string of lane l starts in the round's bytes; the round's bytes last
    __shared__ uint32_t r_src[WAVE];                     // R_LITERAL | byte, or the source position (| R_LATE: it reaches into the round)
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int32_t* row = a.tile_table + (size_t)tile * SQ_LZW_TILE_WORDS;
    const uint32_t total = 3u * a.tile_w * a.tile_h;
    int rc = lzw_range_status(row, a.scans_bytes);       // everything up to the loop is the same in every lane
    if (rc != SQ_LZW_OK) { if (lane == 0) a.status[tile] = rc; return; }
    const unsigned long long off = (unsigned long long)row[0];
    const uint32_t len = (uint32_t)row[1];
    const uint64_t nbits = 8ull * len;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(a.scans);
    const unsigned long long n_words = a.scans_bytes / 4;
    if (nbits < 9) rc = SQ_LZW_TRUNCATED;
    else if (fetch_code(words, n_words, off, 0, 9) != LZW_CLEAR) rc = SQ_LZW_NO_CLEAR;
    if (rc != SQ_LZW_OK) { if (lane == 0) a.status[tile] = rc; return; }
    uint8_t* out = a.chunky + (size_t)tile * total;
    uint64_t seg = 9;                                    // where code 0 of the segment starts
    uint32_t j0 = 0, at = 0;                             // the number of lane 0's code; bytes written
    const uint64_t max_rounds = nbits / 9 + 2;           // a round takes at least one code
    for (uint64_t round = 0; round < max_rounds && at < total; round++) {
        // 1. every lane fetches its code; the round ends before the first code that is not a valid data code
        const uint32_t j = j0 + lane;
        const int width = lzw_code_width(j);
        const uint64_t bit = seg + lzw_code_bit(j);
        const bool have = bit + width <= nbits;
        const uint32_t code = have ? fetch_code(words, n_words, off, bit, width) : LZW_CLEAR;
        const int st = !have ? SQ_LZW_TRUNCATED : code == LZW_CLEAR ? -1 : lzw_code_status(code, j);
        const unsigned long long stops = __ballot(st != SQ_LZW_OK);
        const int n = stops ? __ffsll(stops) - 1 : WAVE;
        bool active = lane < n;
        // 2. lengths: 1 for a literal, the entry's + 1 for a code of an earlier round, and 1 + the length of lane d0 for an
        //    entry of this round, resolved by pointer jumping (len = acc + len[ptr]; six doublings cover a chain of 63)
        const bool literal = code < 256;
        uint32_t acc = 1, src = 0;
        int ptr = -1, d0 = -1;
        bool late = false;
        if (active && !literal) {
            const uint32_t i = code - LZW_FIRST;         // <= j - 1 (lzw_code_status)
            if (i < j0) { acc = (uint32_t)t_len[i] + 1; src = t_pos[i]; late = i + 1 == j0; }   // i + 1 == j0: its last byte is the round's first
            else { d0 = ptr = (int)(i - j0); late = true; }
        }
#pragma unroll
        for (int s = 0; s < 6; s++) {
            const int p = ptr < 0 ? lane : ptr;
            const uint32_t p_acc = __shfl(acc, p, WAVE);
            const int p_ptr = __shfl(ptr, p, WAVE);
            if (ptr >= 0) { acc += p_acc; ptr = p_ptr; }
        }
        // 3. positions: a wave prefix sum; what lies past the tile's end is cut
        const uint32_t mine = active ? acc : 0;
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += up;
        }
        const uint32_t sum = __shfl(incl, WAVE - 1, WAVE);
        const uint32_t bytes = sum < total - at ? sum : total - at;          // of this round
        const uint32_t rel = incl - mine;
        active = active && rel < bytes;
        const uint32_t d_rel = __shfl(rel, d0 < 0 ? lane : d0, WAVE);
        if (d0 >= 0) src = at + d_rel;
        if (active && j < LZW_TABLE_CODES) { t_pos[j] = at + rel; t_len[j] = (uint16_t)acc; }
        r_pos[lane] = active ? rel : bytes;
        r_src[lane] = literal ? (R_LITERAL | code) : (src | (late ? R_LATE : 0u));
        if (lane == 0) r_pos[WAVE] = bytes;
        __syncthreads();
        // 4. strings whose source lies before the round, and literals: all lanes, a byte each
        for (uint32_t b = lane; b < bytes; b += WAVE) {
            int k = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1)
                if (r_pos[k + step] <= b) k += step;                           // k + step <= 63
            const uint32_t e = r_src[k];
            if (e & R_LITERAL) out[at + b] = (uint8_t)e;
            else if (!(e & R_LATE)) out[at + b] = out[(e & R_POS) + (b - r_pos[k])];
        }
        __syncthreads();
        // 5. strings whose source reaches into the round, in order, each by all lanes: the source range [s, s + m) ends at most
        //    one byte into the string itself (the code names the entry being made), and then it repeats with the period p - s
        unsigned long long todo = __ballot(active && late);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1;
            const uint32_t p = at + r_pos[k], m = r_pos[k + 1] - r_pos[k], s = r_src[k] & R_POS, period = p - s;
            if (period >= m) for (uint32_t t = lane; t < m; t += WAVE) out[p + t] = out[s + t];
            else for (uint32_t t = lane; t < m; t += WAVE) out[p + t] = out[s + t % period];
            __syncthreads();
        }
        // 6. what ended the round
        at += bytes;
        if (at >= total) break;
        if (n < WAVE) {
            const int first = __shfl(st, n, WAVE);
            if (first != -1) { rc = first; break; }
            seg = __shfl((unsigned long long)(bit + width), n, WAVE);          // behind the Clear
            j0 = 0;
        } else {
            j0 += WAVE;
        }
    }
    if (rc == SQ_LZW_OK && at < total) rc = SQ_LZW_TRUNCATED;
    if (lane == 0) a.status[tile] = rc;
}

// 12 chunky bytes (four pixels) at p, which is 4-byte aligned
__device__ __forceinline__ void load4px(const uint8_t* p, uint8_t px[12]) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t v = q[i];
#pragma unroll
        for (int k = 0; k < 4; k++) px[4 * i + k] = (uint8_t)(v >> (8 * k));
    }
}

__global__ __launch_bounds__(PLN_THREADS) void lzw_planes_kernel(LzwArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), w = a.tile_w;
    const long long rows = (long long)a.n_tiles * a.tile_h;
    const size_t plane = (size_t)w * a.tile_h;
    const int chunk = (w + WAVE - 1) / WAVE;              // pixels of a row per lane
    const int x0 = lane * chunk < w ? lane * chunk : w, x1 = x0 + chunk < w ? x0 + chunk : w;
    constexpr int ROWS = PLN_THREADS / WAVE;
    for (long long r = (long long)blockIdx.x * ROWS + (threadIdx.x / WAVE); r < rows; r += (long long)gridDim.x * ROWS) {   // the same in a wave
        const int tile = (int)(r / a.tile_h), y = (int)(r % a.tile_h);
        uint8_t* dst = a.planes + (size_t)tile * 3 * plane + (size_t)y * w;
        if (a.status[tile] != SQ_LZW_OK) {                // the planes of a failing tile are zero
            for (int x = x0; x < x1; x++) dst[x] = dst[plane + x] = dst[2 * plane + x] = 0;
            continue;
        }
        const uint8_t* src = (a.compression == 1 ? a.scans + a.tile_table[(size_t)tile * SQ_LZW_TILE_WORDS] : a.chunky + (size_t)tile * 3 * plane)
                             + (size_t)y * w * 3;
        const bool vec = (w % (4 * WAVE)) == 0 && ((uintptr_t)src & 3) == 0;      // whole groups of four pixels, dword loads and stores
        uint32_t c0 = 0, c1 = 0, c2 = 0;                  // the channels' values left of this lane's pixels
        if (a.predictor == 2) {
            uint32_t s0 = 0, s1 = 0, s2 = 0;
            if (vec) {
                for (int x = x0; x < x1; x += 4) {
                    uint8_t px[12];
                    load4px(src + 3 * x, px);
#pragma unroll
                    for (int k = 0; k < 4; k++) { s0 += px[3 * k]; s1 += px[3 * k + 1]; s2 += px[3 * k + 2]; }
                }
            } else {
                for (int x = x0; x < x1; x++) { s0 += src[3 * x]; s1 += src[3 * x + 1]; s2 += src[3 * x + 2]; }
            }
            // two scans: R and G as 16-bit fields of one word (64 lanes of at most 255 each stay below 2^16), B alone
            const uint32_t rg0 = (s0 & 255u) | ((s1 & 255u) << 16), b0 = s2 & 255u;
            uint32_t rg = rg0, bb = b0;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t u = __shfl_up(rg, o, WAVE), v = __shfl_up(bb, o, WAVE);
                if (lane >= o) { rg += u; bb += v; }
            }
            rg -= rg0; bb -= b0;
            c0 = rg & 255u; c1 = (rg >> 16) & 255u; c2 = bb & 255u;
        }
        const uint32_t keep = a.predictor == 2 ? 255u : 0u;                      // predictor 1: a value is the byte itself
        if (vec) {
            for (int x = x0; x < x1; x += 4) {
                uint8_t px[12];
                load4px(src + 3 * x, px);
                uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    c0 = ((c0 & keep) + px[3 * k]) & 255u; c1 = ((c1 & keep) + px[3 * k + 1]) & 255u; c2 = ((c2 & keep) + px[3 * k + 2]) & 255u;
                    o0 |= c0 << (8 * k); o1 |= c1 << (8 * k); o2 |= c2 << (8 * k);
                }
                *reinterpret_cast<uint32_t*>(dst + x) = o0;
                *reinterpret_cast<uint32_t*>(dst + plane + x) = o1;
                *reinterpret_cast<uint32_t*>(dst + 2 * plane + x) = o2;
            }
        } else {
            for (int x = x0; x < x1; x++) {
                c0 = ((c0 & keep) + src[3 * x]) & 255u; c1 = ((c1 & keep) + src[3 * x + 1]) & 255u; c2 = ((c2 & keep) + src[3 * x + 2]) & 255u;
                dst[x] = (uint8_t)c0; dst[plane + x] = (uint8_t)c1; dst[2 * plane + x] = (uint8_t)c2;
            }
        }
    }
}

bool shape_ok(const char* name, int n_tiles, int tile_w, int tile_h, int compression) {
    if (!(tile_w >= 16 && tile_w <= SQ_JPEG_MAX_TILE && tile_h >= 16 && tile_h <= SQ_JPEG_MAX_TILE && !(tile_w & 15) && !(tile_h & 15))) {
        sq_set_error("%s: tiles of %d x %d pixels: extents must be multiples of 16 in 16..%d", name, tile_w, tile_h, SQ_JPEG_MAX_TILE);
        return false;
    }
    if (n_tiles < 1 || n_tiles > (1 << 20)) {
        sq_set_error("%s: n_tiles = %d, must be in 1..%d", name, n_tiles, 1 << 20);
        return false;
    }
    if (compression != 1 && compression != 5) {
        sq_set_error("%s: compression = %d: 5 (LZW) or 1 (none)", name, compression);
        return false;
    }
    return true;
}

struct Layout { size_t chunky, tables, total; };

Layout workspace_layout(int n_tiles, int tile_w, int tile_h, int compression) {
    Layout l;
    size_t at = 0;
    l.chunky = at; at += compression == 5 ? sq_align_up((size_t)n_tiles * 3 * tile_w * tile_h, 256) : 0;
    l.tables = at; at += compression == 5 ? sq_align_up((size_t)n_tiles * LZW_TABLE_CODES * sizeof(LzwEntry), 256) : 256;
    l.total = at;
    return l;
}

}  // namespace

extern "C" size_t sq_lzw_workspace_bytes(int n_tiles, int tile_w, int tile_h, int compression) {
    if (!shape_ok("sq_lzw_workspace_bytes", n_tiles, tile_w, tile_h, compression)) return 0;
    return workspace_layout(n_tiles, tile_w, tile_h, compression).total;
}

extern "C" int sq_lzw_decode_tiles(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles, int tile_w, int tile_h,
                                   int compression, int predictor, int mode, uint8_t* planes, int32_t* status, void* workspace,
                                   size_t workspace_bytes, sq_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!shape_ok("sq_lzw_decode_tiles", n_tiles, tile_w, tile_h, compression)) return SQ_ERR_ARG;
    SQ_REQUIRE(predictor == 1 || predictor == 2, "sq_lzw_decode_tiles: predictor = %d: 1 (none) or 2 (horizontal differencing)", predictor);
    SQ_REQUIRE(mode == SQ_LZW_MODE_WAVE || mode == SQ_LZW_MODE_LANE, "sq_lzw_decode_tiles: mode = %d: SQ_LZW_MODE_WAVE (0) or SQ_LZW_MODE_LANE (1)", mode);
    SQ_REQUIRE(scans && tile_table && planes && status && workspace, "sq_lzw_decode_tiles: a null pointer");
    SQ_REQUIRE(scans_bytes >= 16 && scans_bytes % 16 == 0 && scans_bytes <= 0x7FFFFFF0ull,
               "sq_lzw_decode_tiles: scans of %zu bytes: a multiple of 16 in 16..2^31-16", scans_bytes);
    SQ_REQUIRE(((uintptr_t)scans & 15) == 0 && ((uintptr_t)planes & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tile_table & 3) == 0 &&
               ((uintptr_t)status & 3) == 0, "sq_lzw_decode_tiles: planes, tile_table and status must be 4-byte, scans and the workspace 16-byte aligned");
    SQ_REQUIRE_WORKSPACE("sq_lzw_decode_tiles", workspace_bytes, sq_lzw_workspace_bytes(n_tiles, tile_w, tile_h, compression));
    const Layout l = workspace_layout(n_tiles, tile_w, tile_h, compression);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    LzwArgs a;
    a.scans = scans; a.scans_bytes = scans_bytes; a.tile_table = tile_table; a.n_tiles = n_tiles;
    a.tile_w = tile_w; a.tile_h = tile_h; a.compression = compression; a.predictor = predictor;
    a.chunky = ws + l.chunky; a.tables = reinterpret_cast<LzwEntry*>(ws + l.tables);
    a.planes = planes; a.status = status;
    a.lanes = 1;
    while (a.lanes < WAVE && (n_tiles + a.lanes - 1) / a.lanes > LANE_MAX_WAVES) a.lanes *= 2;
    const double tile_bytes = (double)n_tiles * 3 * tile_w * tile_h;
    char name[96];
    {   // one profiling bracket per launch
        SqProf prof(stream);
        if (compression == 5 && mode == SQ_LZW_MODE_WAVE) {
            if (prof.on()) { snprintf(name, sizeof(name), "lzw_wave_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)scans_bytes + 2.0 * tile_bytes); }
            hipLaunchKernelGGL(lzw_wave_kernel, dim3((unsigned)n_tiles), dim3(WAVE), 0, stream, a);
        } else {
            if (prof.on()) { snprintf(name, sizeof(name), "lzw_lane_c%d_n%d_%dx%d", compression, n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)scans_bytes + 2.0 * tile_bytes); }
            hipLaunchKernelGGL(lzw_lane_kernel, dim3((unsigned)((n_tiles + a.lanes - 1) / a.lanes)), dim3(WAVE), 0, stream, a);
        }
        SQ_LAUNCH_CHECK();
    }
    const long long rows = (long long)n_tiles * tile_h;
    const long long want = (rows + PLN_THREADS / WAVE - 1) / (PLN_THREADS / WAVE);
    SqProf prof(stream);
    if (prof.on()) { snprintf(name, sizeof(name), "lzw_planes_p%d_n%d_%dx%d", predictor, n_tiles, tile_w, tile_h); prof.begin(name, 0.0, 2.0 * tile_bytes); }
    hipLaunchKernelGGL(lzw_planes_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(PLN_THREADS), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
