// JPEG 2000 tiles of an Aperio SVS level (compression 33003 / 33005) -> the planes sq_jpeg_compose_regions reads
// (include/sequoia_hip.h, "JPEG 2000 tiles").  Four kernels: packets (one lane per tile: a packet walk is serial, so up to
// PKT_MAX_WAVES tiles every lane has a wave to itself, as the JPEG entropy kernel does), code-blocks (one wave per block: the
// bit-plane decoder is one serial chain of MQ decisions, so lane 0 decodes while the block's doubled samples, its flags, the
// contexts and the MQ table sit in LDS -- 21 KiB a block, seven blocks per CU, nothing in scratch -- and all 64 lanes clear
// that state before and dequantise it into the component plane afterwards), inverse wavelet (one workgroup per
// tile-component, a barrier between lifting steps, planes in the workspace) and the plane writer (four pixels per thread).
// The arithmetic is j2k_core.h's, which the host check program compiles too.
#include "sq_common.h"
#pragma clang fp contract(off)      // the whole file: the 9/7 lifting and the component transform round every product and sum
#include "j2k_core.h"
#include <stdio.h>

namespace {

constexpr int PKT_THREADS = 64;
constexpr int PKT_MAX_WAVES = 4096;
constexpr int BLK_THREADS = 64;
constexpr int DWT_THREADS = 512;
constexpr int PLN_THREADS = 256;

__constant__ uint32_t MQ_TABLE[J2K_MQ_STATES] = J2K_MQ_TABLE_INIT;

struct J2kArgs {
    const uint8_t* streams; unsigned long long streams_bytes;
    const int32_t* tile_table; int n_tiles;
    int lanes;                           // tiles per wave of the packet kernel
    const uint8_t* sets; int n_sets;
    int tile_w, tile_h;
    J2kCounts cap;
    J2kTile* tiles; J2kBand* bands; J2kBlock* blocks; J2kNode* nodes; uint8_t* gather;
    int32_t* coef; int32_t* tmp;         // [n_tiles][3][tile_h][tile_w]
    uint8_t* planes; int32_t* status;
};

__global__ __launch_bounds__(PKT_THREADS) void j2k_packets_kernel(J2kArgs a) {
    const int tile = blockIdx.x * a.lanes + threadIdx.x;
    if ((int)threadIdx.x >= a.lanes || tile >= a.n_tiles) return;
    J2kTile* T = a.tiles + tile;
    const int rc = j2k_tile_packets(a.sets, a.n_sets, a.tile_table + (size_t)tile * SQ_J2K_TILE_WORDS, a.streams, a.streams_bytes, a.tile_w, a.tile_h,
                                    &a.cap, T, a.bands + (size_t)tile * a.cap.bands, a.blocks + (size_t)tile * a.cap.blocks,
                                    a.nodes + (size_t)tile * a.cap.nodes, a.gather);
    T->status = rc;
    a.status[tile] = rc;
}

__global__ __launch_bounds__(BLK_THREADS) void j2k_blocks_kernel(J2kArgs a) {
    __shared__ uint32_t coef[J2K_BLOCK_MAX * J2K_BLOCK_MAX];
    __shared__ uint8_t flags[J2K_FLAG_BYTES];
    __shared__ uint8_t cx[32];
    __shared__ uint32_t table[J2K_MQ_STATES];
    const int tile = (int)(blockIdx.x / (unsigned)a.cap.blocks), b = (int)(blockIdx.x % (unsigned)a.cap.blocks);
    const J2kTile* T = a.tiles + tile;
    if (T->status != SQ_J2K_OK || b >= T->n_blocks) return;               // the same for the whole wave
    const J2kBlock K = a.blocks[(size_t)tile * a.cap.blocks + b];
    const int w = K.w, h = K.h, t = threadIdx.x;
    if (!K.included || K.passes == 0 || w < 1 || h < 1 || w > J2K_BLOCK_MAX || h > J2K_BLOCK_MAX) return;   // the planes were cleared
    if ((unsigned long long)K.off + K.len > a.streams_bytes || K.x + w > a.tile_w || K.y + h > a.tile_h) return;
    for (int i = t; i < w * h; i += BLK_THREADS) coef[i] = 0;
    for (int i = t; i < (w + 2) * (h + 2); i += BLK_THREADS) flags[i] = 0;
    if (t < J2K_MQ_STATES) table[t] = MQ_TABLE[t];
    __syncthreads();
    if (t == 0) j2k_block_decode(&K, (T->gathered ? a.gather : a.streams) + K.off, coef, flags, cx, table);
    __syncthreads();
    int32_t* plane = a.coef + ((size_t)tile * 3 + K.comp) * a.tile_w * a.tile_h;
    for (int i = t; i < w * h; i += BLK_THREADS)
        plane[(size_t)(K.y + i / w) * a.tile_w + K.x + i % w] = j2k_dequant(coef[i], T->reversible, K.step);
}

__global__ __launch_bounds__(DWT_THREADS) void j2k_idwt_kernel(J2kArgs a) {
    const int tile = blockIdx.x / 3, c = blockIdx.x % 3;
    const J2kTile* T = a.tiles + tile;
    if (T->status != SQ_J2K_OK) return;
    const size_t at = ((size_t)tile * 3 + c) * a.tile_w * a.tile_h;
    const int cw = c == 0 ? a.tile_w : (a.tile_w + T->dx - 1) / T->dx;
    j2k_idwt(cw, a.tile_h, T->levels, T->reversible, a.coef + at, a.tmp + at, a.tile_w, (int)threadIdx.x, DWT_THREADS, [] { __syncthreads(); });
}

__global__ __launch_bounds__(PLN_THREADS) void j2k_planes_kernel(J2kArgs a) {
    const int groups = a.tile_w / 4;
    const size_t plane = (size_t)a.tile_w * a.tile_h;
    const long long total = (long long)a.n_tiles * a.tile_h * groups;
    for (long long i = (long long)blockIdx.x * PLN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PLN_THREADS) {
        const int gx = (int)(i % groups);
        const long long ty = i / groups;
        const int y = (int)(ty % a.tile_h), tile = (int)(ty / a.tile_h);
        const J2kTile* T = a.tiles + tile;
        uint32_t out[3] = {0, 0, 0};
        if (T->status == SQ_J2K_OK) {
            const int32_t* c0 = a.coef + (size_t)tile * 3 * plane + (size_t)y * a.tile_w;
            const int dx = T->dx;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = 4 * gx + j;
                uint8_t px[3];
                j2k_pixel(c0[x], c0[plane + x / dx], c0[2 * plane + x / dx], T->reversible, T->mct, px);
                out[0] |= (uint32_t)px[0] << (8 * j); out[1] |= (uint32_t)px[1] << (8 * j); out[2] |= (uint32_t)px[2] << (8 * j);
            }
        }
        uint8_t* dst = a.planes + (size_t)tile * 3 * plane + (size_t)y * a.tile_w + 4 * gx;
#pragma unroll
        for (int c = 0; c < 3; c++) *reinterpret_cast<uint32_t*>(dst + c * plane) = out[c];
    }
}

bool extent_ok(const char* name, int tile_w, int tile_h) {
    if (tile_w >= 16 && tile_w <= SQ_JPEG_MAX_TILE && tile_h >= 16 && tile_h <= SQ_JPEG_MAX_TILE && !(tile_w & 15) && !(tile_h & 15)) return true;
    sq_set_error("%s: tiles of %d x %d pixels: extents must be multiples of 16 in 16..%d", name, tile_w, tile_h, SQ_JPEG_MAX_TILE);
    return false;
}

bool caps_ok(const char* name, int n_tiles, int max_blocks, int max_nodes, int max_bands) {
    if (n_tiles >= 1 && n_tiles <= (1 << 24) && max_blocks >= 1 && max_blocks <= (1 << 20) && max_nodes >= 1 && max_nodes <= (1 << 22) &&
        max_bands >= 1 && max_bands <= (1 << 20) && (long long)n_tiles * max_blocks < (1ll << 31)) return true;
    sq_set_error("%s: n_tiles = %d, max_blocks = %d, max_nodes = %d, max_bands = %d: n_tiles in 1..2^24, the maxima in 1..2^20, 1..2^22 and "
                 "1..2^20, n_tiles x max_blocks below 2^31", name, n_tiles, max_blocks, max_nodes, max_bands);
    return false;
}

struct Layout { size_t tiles, bands, blocks, nodes, gather, coef, tmp, total; };

Layout workspace_layout(int n_tiles, int tile_w, int tile_h, int max_blocks, int max_nodes, int max_bands, size_t streams_bytes) {
    Layout l;
    size_t at = 0;
    l.tiles = at; at += sq_align_up((size_t)n_tiles * sizeof(J2kTile), 256);
    l.bands = at; at += sq_align_up((size_t)n_tiles * max_bands * sizeof(J2kBand), 256);
    l.blocks = at; at += sq_align_up((size_t)n_tiles * max_blocks * sizeof(J2kBlock), 256);
    l.nodes = at; at += sq_align_up((size_t)n_tiles * max_nodes * sizeof(J2kNode), 256);
    l.gather = at; at += sq_align_up(streams_bytes, 256);
    l.coef = at; at += sq_align_up((size_t)n_tiles * 3 * tile_w * tile_h * 4, 256);
    l.tmp = at; at += sq_align_up((size_t)n_tiles * 3 * tile_w * tile_h * 4, 256);
    l.total = at;
    return l;
}

}  // namespace

extern "C" int sq_j2k_layout(const uint8_t* param_set, int tile_w, int tile_h, int32_t* counts) {
    SQ_REQUIRE(param_set && counts, "sq_j2k_layout: a null pointer");
    if (!extent_ok("sq_j2k_layout", tile_w, tile_h)) return SQ_ERR_ARG;
    J2kParams P;
    SQ_REQUIRE(j2k_params_load(param_set, tile_w, tile_h, &P), "sq_j2k_layout: a field of the parameter set is outside its range "
               "(include/sequoia_hip.h, \"JPEG 2000 tiles\")");
    J2kCounts n;
    j2k_layout(&P, &n, nullptr, nullptr, nullptr, nullptr, nullptr);
    counts[0] = n.blocks; counts[1] = n.nodes; counts[2] = n.bands;
    return SQ_OK;
}

extern "C" size_t sq_j2k_workspace_bytes(int n_tiles, int tile_w, int tile_h, int max_blocks, int max_nodes, int max_bands, size_t streams_bytes) {
    if (!extent_ok("sq_j2k_workspace_bytes", tile_w, tile_h) || !caps_ok("sq_j2k_workspace_bytes", n_tiles, max_blocks, max_nodes, max_bands)) return 0;
    if (streams_bytes < 16 || streams_bytes % 16 || streams_bytes > 0x7FFFFFF0ull) {
        sq_set_error("sq_j2k_workspace_bytes: streams of %zu bytes: a multiple of 16 in 16..2^31-16", streams_bytes);
        return 0;
    }
    return workspace_layout(n_tiles, tile_w, tile_h, max_blocks, max_nodes, max_bands, streams_bytes).total;
}

extern "C" int sq_j2k_decode_tiles(const uint8_t* streams, size_t streams_bytes, const int32_t* tile_table, int n_tiles, const uint8_t* param_sets,
                                   int n_param_sets, int tile_w, int tile_h, int max_blocks, int max_nodes, int max_bands, uint8_t* planes,
                                   int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!extent_ok("sq_j2k_decode_tiles", tile_w, tile_h) || !caps_ok("sq_j2k_decode_tiles", n_tiles, max_blocks, max_nodes, max_bands)) return SQ_ERR_ARG;
    SQ_REQUIRE(n_param_sets >= 1 && n_param_sets <= (1 << 24), "sq_j2k_decode_tiles: n_param_sets = %d, must be in 1..%d", n_param_sets, 1 << 24);
    SQ_REQUIRE(streams && tile_table && param_sets && planes && status && workspace, "sq_j2k_decode_tiles: a null pointer");
    SQ_REQUIRE(streams_bytes >= 16 && streams_bytes % 16 == 0 && streams_bytes <= 0x7FFFFFF0ull,
               "sq_j2k_decode_tiles: streams of %zu bytes: a multiple of 16 in 16..2^31-16", streams_bytes);
    SQ_REQUIRE(((uintptr_t)planes & 3) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tile_table & 3) == 0 && ((uintptr_t)status & 3) == 0,
               "sq_j2k_decode_tiles: planes, tile_table and status must be 4-byte, the workspace 16-byte aligned");
    SQ_REQUIRE_WORKSPACE("sq_j2k_decode_tiles", workspace_bytes,
                         sq_j2k_workspace_bytes(n_tiles, tile_w, tile_h, max_blocks, max_nodes, max_bands, streams_bytes));
    const Layout l = workspace_layout(n_tiles, tile_w, tile_h, max_blocks, max_nodes, max_bands, streams_bytes);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    J2kArgs a;
    a.streams = streams; a.streams_bytes = streams_bytes; a.tile_table = tile_table; a.n_tiles = n_tiles;
    a.sets = param_sets; a.n_sets = n_param_sets; a.tile_w = tile_w; a.tile_h = tile_h;
    a.cap.blocks = max_blocks; a.cap.nodes = max_nodes; a.cap.bands = max_bands;
    a.tiles = reinterpret_cast<J2kTile*>(ws + l.tiles); a.bands = reinterpret_cast<J2kBand*>(ws + l.bands);
    a.blocks = reinterpret_cast<J2kBlock*>(ws + l.blocks); a.nodes = reinterpret_cast<J2kNode*>(ws + l.nodes);
    a.gather = ws + l.gather; a.coef = reinterpret_cast<int32_t*>(ws + l.coef); a.tmp = reinterpret_cast<int32_t*>(ws + l.tmp);
    a.planes = planes; a.status = status;
    a.lanes = 1;
    while (a.lanes < PKT_THREADS && (n_tiles + a.lanes - 1) / a.lanes > PKT_MAX_WAVES) a.lanes *= 2;
    const size_t coef_bytes = (size_t)n_tiles * 3 * tile_w * tile_h * 4;
    char name[96];
    SQ_HIP_CHECK(hipMemsetAsync(a.coef, 0, coef_bytes, stream));          // a block that no packet names writes nothing
    {   // one profiling bracket per launch
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "j2k_packets_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)streams_bytes); }
        hipLaunchKernelGGL(j2k_packets_kernel, dim3((unsigned)((n_tiles + a.lanes - 1) / a.lanes)), dim3(PKT_THREADS), 0, stream, a);
        SQ_LAUNCH_CHECK();
    }
    {
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "j2k_blocks_n%d_b%d", n_tiles, max_blocks); prof.begin(name, 0.0, (double)streams_bytes + (double)coef_bytes); }
        hipLaunchKernelGGL(j2k_blocks_kernel, dim3((unsigned)((long long)n_tiles * max_blocks)), dim3(BLK_THREADS), 0, stream, a);
        SQ_LAUNCH_CHECK();
    }
    {
        SqProf prof(stream);
        if (prof.on()) { snprintf(name, sizeof(name), "j2k_idwt_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, 20.0 * (double)coef_bytes); }
        hipLaunchKernelGGL(j2k_idwt_kernel, dim3((unsigned)(3 * n_tiles)), dim3(DWT_THREADS), 0, stream, a);
        SQ_LAUNCH_CHECK();
    }
    const long long total = (long long)n_tiles * tile_h * (tile_w / 4);
    const long long want = (total + PLN_THREADS - 1) / PLN_THREADS;
    SqProf prof(stream);
    if (prof.on()) { snprintf(name, sizeof(name), "j2k_planes_n%d_%dx%d", n_tiles, tile_w, tile_h); prof.begin(name, 0.0, (double)coef_bytes + (double)n_tiles * 3 * tile_w * tile_h); }
    hipLaunchKernelGGL(j2k_planes_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(PLN_THREADS), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
