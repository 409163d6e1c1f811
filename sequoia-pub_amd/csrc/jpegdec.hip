// JPEG tiles of a tiled TIFF / SVS level -> RGBA regions on the device (include/sequoia_hip.h, "JPEG tiles").
// Five kernels: table derivation (one thread per Huffman table), entropy decode (one lane per tile; the scan is serial, so a
// wave runs as long as its longest lane -- the caller orders the tiles by scan length -- and lanes are spread over waves), IDCT (column pass and row pass through
// LDS, 32 blocks per workgroup) and composition (four RGBA pixels per thread); and, behind sq_jpeg_decode_tiles_split, the entropy decode
// with one WAVE per tile, whose 64 lanes share the tile's scan (self-synchronising subsequences; what is irregular falls back to the
// serial scan on lane 0, so the bytes are the serial kernel's).  The arithmetic is jpeg_core.h's, which the host check programs compile too.
#include "sq_common.h"
#include "jpeg_core.h"
#include <stdio.h>

namespace {

constexpr int ENT_THREADS = 64;          // one wave: its four derived tables sit in LDS once
constexpr int ENT_MAX_WAVES = SQ_JPEG_WAVE_PER_TILE_MAX;      // 256 CUs x 4 SIMDs x 4: below that many tiles every lane has a wave to itself
constexpr int IDCT_BLOCKS = 32, IDCT_THREADS = 256;
constexpr int COEF_STRIDE = 66;          // int16 per staged block: 33 dwords, so a column read hits 32 banks
constexpr int WS_STRIDE = 65;            // int32 per block between the passes
constexpr int CMP_THREADS = 256;

__constant__ uint8_t ZIGZAG[64] = SQJ_ZIGZAG_INIT;

struct JpegArgs {
    const SqjChunk* scans; unsigned long long scans_bytes;
    const int32_t* tile_table; int n_tiles;
    int lanes;                           // tiles per wave of the entropy kernel
    const uint8_t* table_sets; int n_sets;
    SqjGeom g;
    SqjHuff* huff;                       // [n_sets][4]
    uint16_t* quant;                     // [n_sets][4][64], natural order
    int16_t* coefs;                      // [n_tiles][g.blocks][64]
    uint8_t* planes; int32_t* status;
};

__global__ void jpeg_tables_kernel(JpegArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_sets * 4) return;
    const uint8_t* set = a.table_sets + (size_t)(t >> 2) * SQ_JPEG_TABLE_SET_BYTES;
    sqj_build_huff(set + SQJ_QUANT_BYTES + (t & 3) * SQJ_HUFF_BYTES, (t & 3) < 2, a.huff + t);
    const uint8_t* q = set + (t & 3) * 128;
    for (int k = 0; k < 64; k++) a.quant[(size_t)t * 64 + sqj_zigzag(k)] = (uint16_t)(q[2 * k] | (q[2 * k + 1] << 8));
}

__global__ __launch_bounds__(ENT_THREADS) void jpeg_entropy_kernel(JpegArgs a) {
    __shared__ SqjHuff lds_huff[4];
    __shared__ uint8_t lds_zigzag[64];
    // a wave executes the union of its lanes' paths and a scan is serial, so the tiles are spread over as many waves as the
    // device holds: a.lanes of the 64 threads decode (1 below ENT_MAX_WAVES tiles), all of them stage the tables
    const int first = blockIdx.x * a.lanes, tile = first + threadIdx.x;
    lds_zigzag[threadIdx.x] = ZIGZAG[threadIdx.x];
    const int set0 = a.tile_table[(size_t)first * SQ_JPEG_TILE_WORDS + 2];              // first < n_tiles by the grid
    if (set0 >= 0 && set0 < a.n_sets) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.huff + (size_t)set0 * 4);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds_huff);
        for (int i = threadIdx.x; i < (int)(4 * sizeof(SqjHuff) / 4); i += ENT_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= a.lanes || tile >= a.n_tiles) return;
    const int32_t* row = a.tile_table + (size_t)tile * SQ_JPEG_TILE_WORDS;
    int rc = sqj_tile_check(row, a.n_sets, a.scans_bytes, a.huff);
    if (rc == SQ_JPEG_OK) {
        // the wave's tables from LDS; a lane of another table set (rare: tiles that carry their own tables) reads global memory
        const SqjHuff* huff = row[2] == set0 ? lds_huff : a.huff + (size_t)row[2] * 4;
        rc = sqj_scan(a.scans, (uint32_t)row[0], (uint32_t)row[0] + (uint32_t)row[1], &a.g, huff, lds_zigzag, row[4], row[3],
                      a.coefs + (size_t)tile * a.g.blocks * 64);
    }
    a.status[tile] = rc;
}

// ---- the split entropy decode: one wave per tile, its 64 lanes on the tile's scan (jpeg_core.h, "one scan split over the lanes") ----
__device__ __forceinline__ SqjState shfl_up_state(const SqjState& s, int d) {
    SqjState r;
    r.pos = (uint32_t)__shfl_up((int)s.pos, d); r.bit = __shfl_up(s.bit, d); r.blk = __shfl_up(s.blk, d);
    r.k = __shfl_up(s.k, d); r.valid = __shfl_up(s.valid, d);
    return r;
}
__device__ __forceinline__ SqjState shfl_state(const SqjState& s, int lane) {
    SqjState r;
    r.pos = (uint32_t)__shfl((int)s.pos, lane); r.bit = __shfl(s.bit, lane); r.blk = __shfl(s.blk, lane);
    r.k = __shfl(s.k, lane); r.valid = __shfl(s.valid, lane);
    return r;
}
// inclusive sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < ENT_THREADS; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(ENT_THREADS) void jpeg_entropy_split_kernel(JpegArgs a, int sub) {
    __shared__ SqjHuff lds_huff[4];
    __shared__ uint8_t lds_zigzag[64];
    const int tile = blockIdx.x, lane = threadIdx.x;                       // tile < n_tiles by the grid
    const int32_t* row = a.tile_table + (size_t)tile * SQ_JPEG_TILE_WORDS;
    const int checked = sqj_tile_check(row, a.n_sets, a.scans_bytes, a.huff);           // the same on every lane
    lds_zigzag[lane] = ZIGZAG[lane];
    if (checked == SQ_JPEG_OK) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.huff + (size_t)row[2] * 4);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds_huff);
        for (int i = lane; i < (int)(4 * sizeof(SqjHuff) / 4); i += ENT_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    if (checked != SQ_JPEG_OK) {
        if (lane == 0) a.status[tile] = checked;
        return;
    }
    // from here every branch but those inside sqj_sub_run is taken by the whole wave: the conditions come from votes and shuffles
    const uint32_t pos = (uint32_t)row[0], end = pos + (uint32_t)row[1];
    const int sel = row[4], restart = row[3];
    const long long n_sub = ((long long)row[1] + sub - 1) / sub;
    int16_t* coefs = a.coefs + (size_t)tile * a.g.blocks * 64;
    const uint32_t want = (uint32_t)a.g.blocks;
    bool done = false, bad = restart > 0;
    SqjState carry;
    carry.pos = pos; carry.bit = 0; carry.blk = 0; carry.k = 0; carry.valid = 1;
    uint32_t base = 0, pred0 = 0, pred1 = 0, pred2 = 0;
    for (long long first = 0; first < n_sub && !done && !bad; first += ENT_THREADS) {
        const unsigned long long at = (unsigned long long)pos + (unsigned long long)(first + lane) * sub;
        const uint32_t sub_end = (uint32_t)(at + sub < end ? at + sub : end);
        const bool live = first + lane < n_sub;
        const SqjState guess = lane == 0 ? carry : sqj_sub_guess(a.scans, pos, end, (uint32_t)(at < end ? at : end));
        SqjState start = guess;
        SqjSubResult res;
        sqj_sub_run(a.scans, end, &a.g, lds_huff, lds_zigzag, sel, &start, sub_end, false, 0, 0, 0, 0, coefs, &res);
        for (int r = 0; r < ENT_THREADS - 1; r++) {                        // lane r is exact after round r
            const SqjState in = shfl_up_state(res.end, 1);
            const SqjState next = (lane == 0 || !live) ? start : in.valid ? in : guess;      // a lane behind the scan's end has nothing to agree on
            const bool changed = !sqj_state_same(next, start);
            if (!__any(changed)) break;
            if (changed) {
                start = next;
                sqj_sub_run(a.scans, end, &a.g, lds_huff, lds_zigzag, sel, &start, sub_end, false, 0, 0, 0, 0, coefs, &res);
            }
        }
        const uint32_t blocks_in = wave_scan((uint32_t)res.blocks, lane), s0 = wave_scan(res.dc0, lane), s1 = wave_scan(res.dc1, lane),
                       s2 = wave_scan(res.dc2, lane);
        const bool reached = base + blocks_in >= want;                     // the scan's last block ends in this lane or before it
        const unsigned long long reached_mask = __ballot(reached);
        const int last = reached_mask ? __builtin_ctzll(reached_mask) : ENT_THREADS - 1;
        if (__any(lane <= last && !reached && !res.end.valid)) bad = true;
        if (reached_mask) {
            done = true;
            if (base + (uint32_t)__shfl((int)blocks_in, last) > want) bad = true;
        }
        if (bad) break;
        SqjSubResult w;
        w.rc = SQ_JPEG_OK;
        if (lane <= last)
            sqj_sub_run(a.scans, end, &a.g, lds_huff, lds_zigzag, sel, &start, sub_end, true, (int)(base + blocks_in - (uint32_t)res.blocks),
                        pred0 + s0 - res.dc0, pred1 + s1 - res.dc1, pred2 + s2 - res.dc2, coefs, &w);
        if (__any(w.rc != SQ_JPEG_OK)) bad = true;
        const SqjState reached_state = shfl_state(res.end, ENT_THREADS - 1);
        if (!done && sqj_state_same(reached_state, carry)) bad = true;      // a marker in the scan: no lane can pass it, the serial scan says why
        carry = reached_state;
        base += (uint32_t)__shfl((int)blocks_in, ENT_THREADS - 1);
        pred0 += (uint32_t)__shfl((int)s0, ENT_THREADS - 1);
        pred1 += (uint32_t)__shfl((int)s1, ENT_THREADS - 1);
        pred2 += (uint32_t)__shfl((int)s2, ENT_THREADS - 1);
    }
    int rc = SQ_JPEG_OK;
    if (!done || bad) {                  // anything irregular: the serial scan's status and coefficients
        __syncthreads();                 // the lanes' stores are behind the zeros
        u32x4* z = reinterpret_cast<u32x4*>(coefs);
        const u32x4 zero = {0, 0, 0, 0};
        for (int i = lane; i < a.g.blocks * 8; i += ENT_THREADS) z[i] = zero;
        __syncthreads();                 // and the zeros behind lane 0's stores
        if (lane == 0) rc = sqj_scan(a.scans, pos, end, &a.g, lds_huff, lds_zigzag, sel, restart, coefs);
    }
    if (lane == 0) a.status[tile] = rc;
}

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(JpegArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t cbuf[IDCT_BLOCKS * COEF_STRIDE];
    __shared__ int32_t ws[IDCT_BLOCKS * WS_STRIDE];
    const long long total = (long long)a.n_tiles * a.g.blocks;
    const long long base = (long long)blockIdx.x * IDCT_BLOCKS;
    const int t = threadIdx.x;
    {   // 32 blocks x 128 bytes, 16 bytes per thread: thread t holds row t % 8 of block t / 8
        const long long gblk = base + (t >> 3);
        u32x4 v = {0, 0, 0, 0};
        if (gblk < total) v = *reinterpret_cast<const u32x4*>(a.coefs + (size_t)gblk * 64 + (t & 7) * 8);
        uint32_t* dst = reinterpret_cast<uint32_t*>(cbuf + (t >> 3) * COEF_STRIDE + (t & 7) * 8);
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
    }
    __syncthreads();
    const int blk = t & 31, lane8 = t >> 5;             // column in the first pass, row in the second
    const long long gblk = base + blk;
    const bool live = gblk < total;
    int tile = 0, c = 0, bx = 0, by = 0;
    if (live) {
        tile = (int)(gblk / a.g.blocks);
        int bi = (int)(gblk % a.g.blocks);
        const int yb = (a.g.tile_w / 8) * (a.g.tile_h / 8), cb = (a.g.cw / 8) * (a.g.ch / 8);
        if (bi >= yb) { c = 1 + (bi - yb) / cb; bi = (bi - yb) % cb; }
        const int bw = (c == 0 ? a.g.tile_w : a.g.cw) / 8;
        bx = bi % bw; by = bi / bw;
    }
    {
        int32_t x[8], y[8];
        const int32_t* row = a.tile_table + (size_t)tile * SQ_JPEG_TILE_WORDS;
        const int set = row[2];
        const bool have_q = live && set >= 0 && set < a.n_sets;            // no table set: zeros, a flat block
        const uint16_t* q = a.quant + ((size_t)(have_q ? set : 0) * 4 + ((row[4] >> (4 * c)) & 3)) * 64;
#pragma unroll
        for (int r = 0; r < 8; r++) x[r] = have_q ? sqj_dequant(cbuf[blk * COEF_STRIDE + r * 8 + lane8], q[r * 8 + lane8]) : 0;
        sqj_idct_1d(x, y, 11);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[blk * WS_STRIDE + r * 8 + lane8] = y[r];
    }
    __syncthreads();
    if (!live) return;
    int32_t x[8], y[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ws[blk * WS_STRIDE + lane8 * 8 + j];
    sqj_idct_1d(x, y, 18);
    const int pw = c == 0 ? a.g.tile_w : a.g.cw;
    uint8_t* plane = a.planes + (size_t)tile * a.g.plane_bytes
                   + (c == 0 ? 0 : (size_t)a.g.tile_w * a.g.tile_h + (size_t)(c - 1) * a.g.cw * a.g.ch);
    u32x2 out;
    out[0] = sqj_sample(y[0]) | (sqj_sample(y[1]) << 8) | (sqj_sample(y[2]) << 16) | ((uint32_t)sqj_sample(y[3]) << 24);
    out[1] = sqj_sample(y[4]) | (sqj_sample(y[5]) << 8) | (sqj_sample(y[6]) << 16) | ((uint32_t)sqj_sample(y[7]) << 24);
    *reinterpret_cast<u32x2*>(plane + (size_t)(by * 8 + lane8) * pw + bx * 8) = out;       // 32 lanes: 256 adjacent bytes
}

struct ComposeArgs {
    const uint8_t* planes; int n_slots; SqjGeom g; int transform;
    const int32_t* tile_slot; int tiles_x, tiles_y, level_w, level_h;
    const int32_t* regions; int k, h, w, groups;      // groups of four pixels per row
    uint8_t* rgba;
};

__device__ __forceinline__ uint32_t compose_pixel(const ComposeArgs& a, long long X, long long Y) {
    if (X < 0 || X >= a.level_w || Y < 0 || Y >= a.level_h) return 0u;
    const int tx = (int)X / a.g.tile_w, ty = (int)Y / a.g.tile_h;
    if (tx >= a.tiles_x || ty >= a.tiles_y) return 0u;
    const int slot = a.tile_slot[(size_t)ty * a.tiles_x + tx];
    if (slot < 0 || slot >= a.n_slots) return 0u;
    return sqj_pixel(a.planes + (size_t)slot * a.g.plane_bytes, &a.g, (int)X - tx * a.g.tile_w, (int)Y - ty * a.g.tile_h, a.transform);
}

__global__ __launch_bounds__(CMP_THREADS) void jpeg_compose_kernel(ComposeArgs a) {
    const long long total = (long long)a.k * a.h * a.groups;
    for (long long i = (long long)blockIdx.x * CMP_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * CMP_THREADS) {
        const int gx = (int)(i % a.groups);
        const long long ry = i / a.groups;
        const int y = (int)(ry % a.h), r = (int)(ry / a.h);
        const long long X = (long long)a.regions[2 * (size_t)r] + 4 * gx, Y = (long long)a.regions[2 * (size_t)r + 1] + y;
        uint8_t* dst = a.rgba + (((size_t)r * a.h + y) * a.w + 4 * (size_t)gx) * 4;
        if ((a.w & 3) == 0) {
            u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = compose_pixel(a, X + j, Y);
            *reinterpret_cast<u32x4*>(dst) = v;
        } else {
            for (int j = 0; j < 4 && 4 * gx + j < a.w; j++) reinterpret_cast<uint32_t*>(dst)[j] = compose_pixel(a, X + j, Y);
        }
    }
}

bool frame_ok(const char* name, int tile_w, int tile_h, int hs, int vs, SqjGeom* g) {
    if (sqj_geom(tile_w, tile_h, hs, vs, g)) return true;
    sq_set_error("%s: a frame of %d x %d pixels with luma sampling %d x %d: extents must be multiples of 16 in 16..%d and the "
                 "sampling 1 x 1, 2 x 1 or 2 x 2", name, tile_w, tile_h, hs, vs, SQ_JPEG_MAX_TILE);
    return false;
}

size_t huff_bytes(int n_sets) { return sq_align_up((size_t)n_sets * 4 * sizeof(SqjHuff), 256); }
size_t quant_bytes(int n_sets) { return sq_align_up((size_t)n_sets * 4 * 64 * sizeof(uint16_t), 256); }

}  // namespace

extern "C" size_t sq_jpeg_workspace_bytes(int n_tiles, int n_table_sets, int tile_w, int tile_h, int hs, int vs) {
    SqjGeom g;
    if (!frame_ok("sq_jpeg_workspace_bytes", tile_w, tile_h, hs, vs, &g)) return 0;
    if (n_tiles < 1 || n_table_sets < 1) {
        sq_set_error("sq_jpeg_workspace_bytes: n_tiles = %d, n_table_sets = %d, both must be at least 1", n_tiles, n_table_sets);
        return 0;
    }
    return huff_bytes(n_table_sets) + quant_bytes(n_table_sets) + (size_t)n_tiles * g.blocks * 128;
}

extern "C" size_t sq_jpeg_planes_bytes(int n_tiles, int tile_w, int tile_h, int hs, int vs) {
    SqjGeom g;
    if (!frame_ok("sq_jpeg_planes_bytes", tile_w, tile_h, hs, vs, &g)) return 0;
    if (n_tiles < 1) {
        sq_set_error("sq_jpeg_planes_bytes: n_tiles = %d, must be at least 1", n_tiles);
        return 0;
    }
    return (size_t)n_tiles * g.plane_bytes;
}

// both decode entries; sub < 0: the serial entropy kernel, else the split one with subsequences of `sub` bytes
static int decode_tiles(const char* entry, int sub, const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles,
                        const uint8_t* table_sets, int n_table_sets, int tile_w, int tile_h, int hs, int vs,
                        uint8_t* planes, int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    JpegArgs a;
    if (!frame_ok(entry, tile_w, tile_h, hs, vs, &a.g)) return SQ_ERR_ARG;
    SQ_REQUIRE(n_tiles >= 1 && n_tiles <= (1 << 24), "%s: n_tiles = %d, must be in 1..%d", entry, n_tiles, 1 << 24);
    SQ_REQUIRE(n_table_sets >= 1 && n_table_sets <= (1 << 24), "%s: n_table_sets = %d, must be in 1..%d", entry, n_table_sets, 1 << 24);
    SQ_REQUIRE(scans && tile_table && table_sets && planes && status && workspace, "%s: a null pointer", entry);
    SQ_REQUIRE(scans_bytes >= 16 && scans_bytes % 16 == 0 && scans_bytes <= 0xFFFFFFF0ull && ((uintptr_t)scans & 15) == 0,
               "%s: scans of %zu bytes at %p: the base must be 16-byte aligned and the size a multiple of 16 in 16..2^32-16",
               entry, scans_bytes, (const void*)scans);
    SQ_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tile_table & 3) == 0 && ((uintptr_t)status & 3) == 0,
               "%s: planes must be 8-byte, the workspace 16-byte, tile_table and status 4-byte aligned", entry);
    SQ_REQUIRE_WORKSPACE(entry, workspace_bytes, sq_jpeg_workspace_bytes(n_tiles, n_table_sets, tile_w, tile_h, hs, vs));
    a.scans = reinterpret_cast<const SqjChunk*>(scans); a.scans_bytes = scans_bytes;
    a.tile_table = tile_table; a.n_tiles = n_tiles; a.table_sets = table_sets; a.n_sets = n_table_sets;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    a.huff = reinterpret_cast<SqjHuff*>(ws);
    a.quant = reinterpret_cast<uint16_t*>(ws + huff_bytes(n_table_sets));
    a.coefs = reinterpret_cast<int16_t*>(ws + huff_bytes(n_table_sets) + quant_bytes(n_table_sets));
    a.planes = planes; a.status = status;
    const size_t coef_bytes = (size_t)n_tiles * a.g.blocks * 128;
    const long long blocks = (long long)n_tiles * a.g.blocks;
    a.lanes = 1;
    while (a.lanes < ENT_THREADS && (n_tiles + a.lanes - 1) / a.lanes > ENT_MAX_WAVES) a.lanes *= 2;
    char name[96];
    SQ_HIP_CHECK(hipMemsetAsync(a.coefs, 0, coef_bytes, stream));        // the entropy lanes write non-zero coefficients only
    {   // one profiling bracket per launch
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "jpeg_tables_s%d", n_table_sets); prof.begin(name, 0.0, (double)n_table_sets * 8000.0); }
        hipLaunchKernelGGL(jpeg_tables_kernel, dim3((unsigned)((n_table_sets * 4 + 63) / 64)), dim3(64), 0, stream, a);
        SQ_LAUNCH_CHECK();
    }
    if (sub < 0) {
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "jpeg_entropy_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)scans_bytes + (double)coef_bytes); }
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((n_tiles + a.lanes - 1) / a.lanes)), dim3(ENT_THREADS), 0, stream, a);
        SQ_LAUNCH_CHECK();
    } else {
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "jpeg_entropy_split_n%d_%dx%d_b%d", n_tiles, tile_w, tile_h, sub); prof.begin(name, 0.0, (double)scans_bytes + (double)coef_bytes); }
        hipLaunchKernelGGL(jpeg_entropy_split_kernel, dim3((unsigned)n_tiles), dim3(ENT_THREADS), 0, stream, a, sub);
        SQ_LAUNCH_CHECK();
    }
    SqProf prof(stream);
    if (prof.on()) { snprintf(name, sizeof(name), "jpeg_idct_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)coef_bytes + (double)n_tiles * a.g.plane_bytes); }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(IDCT_THREADS), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_jpeg_decode_tiles(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles,
                                    const uint8_t* table_sets, int n_table_sets, int tile_w, int tile_h, int hs, int vs,
                                    uint8_t* planes, int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream) {
    return decode_tiles("sq_jpeg_decode_tiles", -1, scans, scans_bytes, tile_table, n_tiles, table_sets, n_table_sets, tile_w, tile_h, hs, vs,
                        planes, status, workspace, workspace_bytes, stream);
}

extern "C" size_t sq_jpeg_split_workspace_bytes(int n_tiles, int n_table_sets, int tile_w, int tile_h, int hs, int vs) {
    return sq_jpeg_workspace_bytes(n_tiles, n_table_sets, tile_w, tile_h, hs, vs);       // the lane states live in registers
}

extern "C" int sq_jpeg_decode_tiles_split(const uint8_t* scans, size_t scans_bytes, const int32_t* tile_table, int n_tiles,
                                          const uint8_t* table_sets, int n_table_sets, int tile_w, int tile_h, int hs, int vs,
                                          uint8_t* planes, int32_t* status, void* workspace, size_t workspace_bytes, int sub_bytes,
                                          sq_stream_t stream) {
    SQ_REQUIRE(sub_bytes == 0 || (sub_bytes >= SQ_JPEG_SPLIT_SUB_MIN && sub_bytes <= SQ_JPEG_SPLIT_SUB_MAX && sub_bytes % 4 == 0),
               "sq_jpeg_decode_tiles_split: sub_bytes = %d, must be a multiple of 4 in %d..%d, or 0 for the default (%d)", sub_bytes,
               SQ_JPEG_SPLIT_SUB_MIN, SQ_JPEG_SPLIT_SUB_MAX, SQ_JPEG_SPLIT_SUB_DEFAULT);
    return decode_tiles("sq_jpeg_decode_tiles_split", sub_bytes ? sub_bytes : SQ_JPEG_SPLIT_SUB_DEFAULT, scans, scans_bytes, tile_table, n_tiles,
                        table_sets, n_table_sets, tile_w, tile_h, hs, vs, planes, status, workspace, workspace_bytes, stream);
}

extern "C" int sq_jpeg_compose_regions(const uint8_t* planes, int n_slots, int tile_w, int tile_h, int hs, int vs, int transform,
                                       const int32_t* tile_slot, int tiles_x, int tiles_y, int level_w, int level_h,
                                       const int32_t* regions, int k, int h, int w, uint8_t* rgba, sq_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ComposeArgs a;
    if (!frame_ok("sq_jpeg_compose_regions", tile_w, tile_h, hs, vs, &a.g)) return SQ_ERR_ARG;
    SQ_REQUIRE(n_slots >= 1 && n_slots <= (1 << 24), "sq_jpeg_compose_regions: n_slots = %d, must be in 1..%d", n_slots, 1 << 24);
    SQ_REQUIRE(level_w >= 1 && level_h >= 1 && level_w <= (1 << 24) && level_h <= (1 << 24),
               "sq_jpeg_compose_regions: a level of %d x %d pixels, extents must be in 1..%d", level_w, level_h, 1 << 24);
    SQ_REQUIRE(tiles_x == (level_w + tile_w - 1) / tile_w && tiles_y == (level_h + tile_h - 1) / tile_h,
               "sq_jpeg_compose_regions: a grid of %d x %d tiles of %d x %d pixels for a level of %d x %d", tiles_x, tiles_y, tile_w, tile_h,
               level_w, level_h);
    SQ_REQUIRE(k >= 0 && k <= (1 << 24) && h >= 1 && w >= 1 && h <= SQ_JPEG_MAX_REGION && w <= SQ_JPEG_MAX_REGION,
               "sq_jpeg_compose_regions: k = %d regions of %d x %d pixels: k in 0..%d, extents in 1..%d", k, w, h, 1 << 24, SQ_JPEG_MAX_REGION);
    if (k == 0) return SQ_OK;
    SQ_REQUIRE(planes && tile_slot && regions && rgba, "sq_jpeg_compose_regions: a null pointer");
    SQ_REQUIRE(((uintptr_t)rgba & 15) == 0 && ((uintptr_t)tile_slot & 3) == 0 && ((uintptr_t)regions & 3) == 0,
               "sq_jpeg_compose_regions: rgba must be 16-byte, tile_slot and regions 4-byte aligned");
    a.planes = planes; a.n_slots = n_slots; a.transform = transform ? 1 : 0;
    a.tile_slot = tile_slot; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.level_w = level_w; a.level_h = level_h;
    a.regions = regions; a.k = k; a.h = h; a.w = w; a.groups = (w + 3) / 4; a.rgba = rgba;
    const long long total = (long long)k * h * a.groups;
    const long long want = (total + CMP_THREADS - 1) / CMP_THREADS;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    SqProf prof(stream);
    if (prof.on()) {
        char name[96];
        snprintf(name, sizeof(name), "jpeg_compose_k%d_%dx%d", k, w, h);
        prof.begin(name, 0.0, (double)k * h * w * 6.0);
    }
    hipLaunchKernelGGL(jpeg_compose_kernel, dim3(grid), dim3(CMP_THREADS), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
