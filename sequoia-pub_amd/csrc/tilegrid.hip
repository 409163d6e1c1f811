// Valid-tile grid of the spatial maps on the device (include/sequoia_hip.h, "Tile grid"): the double loop of
// spatial_vis/visualize.py:174-205 over every grid tile of a slide -- scipy's binary_dilation(iterations=k) of the tile's
// window of the tissue mask, its count against threshold x the window's size -- as ONE launch.  The mask is the array of
// mask.npy, uint8 [mask_w, mask_h] indexed [x, y]; a window is x in [c, c + pm), y in [r, r + pm) clipped to the mask, and
// the dilation sees zeros outside the WINDOW (scipy's border_value = 0 on the slice), so nothing of a neighbouring window
// enters.  The cross is symmetric: the kernels walk the window in the mask's own layout, a "row" of bits is the y run of
// one x, contiguous in memory.
// Two routes, chosen by pm before the launch:
//   packed  pm <= 64   a window row is one machine word of one lane (32 bits up to pm = 32, 64 bits beyond); a window takes
//                      G = 8, 16, 32 or 64 adjacent lanes, so a wave holds 8, 4, 2 or 1 windows; a step of the cross is two
//                      shifts and the words of the lanes above and below; the count is a popcount summed over the G lanes.
//   wide    pm <= 512  one workgroup per window: the window's bits in LDS (512 rows x 16 words = 32 KiB, ONE image: no second
//                      buffer), and every output word straight from it: k steps of the cross are the diamond |dx| + |dy| <= k,
//                      so out(x) = OR over dx of the row x + dx smeared by k - |dx| bits either way.  No barrier per step.
// Every window is independent and every sum is an integer: two calls give the same bytes.  Indexing into the mask is 64-bit.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"

#pragma clang fp contract(off)      // threshold x size is one rounded product, as numpy's

namespace {

constexpr int TG_THREADS = 256;
constexpr int TG_WIDE_WORDS = SQ_TILE_GRID_MAX_WINDOW / 32;       // 32-bit words per row of the LDS image

struct TgArgs {
    const uint8_t* mask;     // [mask_w][mask_h]
    uint8_t* valid;          // [n_col][n_row]
    int32_t* counts;         // or null
    int32_t* sizes;          // or null
    int mask_w, mask_h, n_col, n_row, p, ds, pm, iterations;
    int tiles;               // n_col n_row <= 2^30
    double threshold;
};

// window of grid tile t = i n_row + j: first mask row (x) and bit (y), clipped extents (0 when the origin is beyond the mask)
// (t <= 2^30 and every tile origin is below 2^31, checked before the launch: 32-bit unsigned arithmetic holds them)
__device__ __forceinline__ void tg_window(const TgArgs& a, int t, int& c, int& r, int& wx, int& wy) {
    const uint32_t i = (uint32_t)t / (uint32_t)a.n_row, j = (uint32_t)t - i * (uint32_t)a.n_row;
    const uint32_t cc = i * (uint32_t)a.p / (uint32_t)a.ds, rr = j * (uint32_t)a.p / (uint32_t)a.ds;      // int(col / downsample_factor)
    c = (int)min(cc, (uint32_t)a.mask_w), r = (int)min(rr, (uint32_t)a.mask_h);
    wx = min(a.pm, a.mask_w - c), wy = min(a.pm, a.mask_h - r);
}

__device__ __forceinline__ void tg_emit(const TgArgs& a, int t, int count, int size) {
    a.valid[t] = (uint8_t)((double)count >= a.threshold * (double)size);
    if (a.counts) a.counts[t] = count;
    if (a.sizes) a.sizes[t] = size;
}

__device__ __forceinline__ int tg_popc(uint32_t w) { return __popc(w); }
__device__ __forceinline__ int tg_popc(unsigned long long w) { return __popcll(w); }

// G lanes per window, lane lx of the group holds row c + lx as a word of type W (bit b = mask[c + lx][r + b])
template <int G, typename W>
__global__ __launch_bounds__(TG_THREADS) void tile_grid_packed_kernel(const TgArgs a) {
    const int tid = threadIdx.x, lx = tid & (G - 1);
    const int t = (int)(blockIdx.x * (TG_THREADS / G) + tid / G);
    const bool live = t < a.tiles;                  // a dead group still takes part in the shuffles of its wave
    int c = 0, r = 0, wx = 0, wy = 0;
    if (live) tg_window(a, t, c, r, wx, wy);
    const bool row_in = lx < wx;
    W w = 0;
    if (row_in) {
        const uint8_t* const src = a.mask + (size_t)(c + lx) * (size_t)a.mask_h + (size_t)r;
        for (int b = 0; b < wy; ++b) w |= (W)(src[b] != 0) << b;
    }
    // the bits of a row inside the window; wy = 0 leaves none.  Rows beyond wx stay zero: `keep` is zero there
    const W keep = !row_in || wy == 0 ? (W)0 : (wy >= (int)(8 * sizeof(W)) ? ~(W)0 : (((W)1 << wy) - 1));
    for (int it = 0; it < a.iterations; ++it) {
        W up = __shfl_up(w, 1, G), down = __shfl_down(w, 1, G);
        if (lx == 0) up = 0;
        if (lx == G - 1) down = 0;
        w = (w | (w << 1) | (w >> 1) | up | down) & keep;
    }
    int count = tg_popc(w);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) count += __shfl_xor(count, o, G);
    if (live && lx == 0) tg_emit(a, t, count, wx * wy);
}

// one workgroup per window; bits[x][j]: bit b of word j = mask[c + x][r + 32 j + b]
__global__ __launch_bounds__(TG_THREADS) void tile_grid_wide_kernel(const TgArgs a) {
    __shared__ uint32_t bits[SQ_TILE_GRID_MAX_WINDOW * TG_WIDE_WORDS];
    __shared__ int wave_count[TG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = (int)blockIdx.x;
    int c, r, wx, wy;
    tg_window(a, t, c, r, wx, wy);                  // the same for every thread of the workgroup
    const int words = (wy + 31) >> 5, chunks = (wy + 63) >> 6;            // per row: 32-bit words, 64-lane ballots
    // a wave takes 64 consecutive y of one row: a ballot is two whole words, the bits beyond wy are zero
    for (int item = wave; item < wx * chunks; item += TG_THREADS / 64) {
        const int x = item / chunks, q = item - x * chunks, y = q * 64 + lane;
        const bool on = y < wy && a.mask[(size_t)(c + x) * (size_t)a.mask_h + (size_t)(r + y)] != 0;
        const unsigned long long m = __ballot(on);
        if (lane == 0) {
            bits[x * TG_WIDE_WORDS + 2 * q] = (uint32_t)m;
            if (2 * q + 1 < words) bits[x * TG_WIDE_WORDS + 2 * q + 1] = (uint32_t)(m >> 32);
        }
    }
    __syncthreads();
    const int k = a.iterations;
    const uint32_t last_keep = (wy & 31) ? (1u << (wy & 31)) - 1u : 0xffffffffu;
    int count = 0;
    for (int idx = tid; idx < wx * words; idx += TG_THREADS) {
        const int x = idx / words, j = idx - x * words;
        uint32_t acc = 0;
        for (int dx = -k; dx <= k; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= wx) continue;       // rows outside the window are zero
            const uint32_t* const row = bits + xx * TG_WIDE_WORDS;
            const uint32_t m = row[j], left = j > 0 ? row[j - 1] : 0u, right = j < words - 1 ? row[j + 1] : 0u;
            // the word with its lower neighbour below it, smeared upwards; with its upper neighbour above it, smeared downwards
            unsigned long long lo = ((unsigned long long)m << 32) | left, hi = ((unsigned long long)right << 32) | m;
            const int reach = k - (dx < 0 ? -dx : dx);
            unsigned long long s_up = lo, s_down = hi;
            for (int s = 1; s <= reach; ++s) s_up |= lo << s, s_down |= hi >> s;
            acc |= (uint32_t)(s_up >> 32) | (uint32_t)s_down;
        }
        if (j == words - 1) acc &= last_keep;
        count += __popc(acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int i = 0; i < TG_THREADS / 64; ++i) total += wave_count[i];
        tg_emit(a, t, total, wx * wy);
    }
}

template <int G, typename W>
void tg_launch_packed(const TgArgs& a, hipStream_t stream) {
    constexpr int per_block = TG_THREADS / G;
    hipLaunchKernelGGL((tile_grid_packed_kernel<G, W>), dim3((unsigned)((a.tiles + per_block - 1) / per_block)), dim3(TG_THREADS), 0, stream, a);
}

}  // namespace

static_assert(SQ_TILE_GRID_MAX_WINDOW % 64 == 0 && sizeof(uint32_t) * SQ_TILE_GRID_MAX_WINDOW * TG_WIDE_WORDS + 64 <= 65536,
              "a window's bit image fits the static LDS limit");
static_assert(SQ_TILE_GRID_PACKED_MAX_WINDOW == 64, "the packed route's widest word");

extern "C" int sq_tile_grid_valid(const uint8_t* mask_u8, int mask_w, int mask_h, int n_col, int n_row, int p, int ds, int pm,
                                  int iterations, double threshold, uint8_t* valid, int32_t* counts, int32_t* sizes,
                                  sq_stream_t stream_) {
    SQ_REQUIRE(mask_w >= 1 && mask_w <= SQ_TILE_GRID_MAX_DIM && mask_h >= 1 && mask_h <= SQ_TILE_GRID_MAX_DIM,
               "tile_grid_valid: mask of %d x %d: both extents must be in 1..%d", mask_w, mask_h, SQ_TILE_GRID_MAX_DIM);
    SQ_REQUIRE((long long)mask_w * mask_h <= (1ll << 30), "tile_grid_valid: mask of %d x %d: more than 2^30 elements", mask_w, mask_h);
    SQ_REQUIRE(n_col >= 1 && n_row >= 1 && (long long)n_col * n_row <= (1ll << 30),
               "tile_grid_valid: grid of %d x %d tiles: both extents at least 1 and at most 2^30 tiles", n_col, n_row);
    SQ_REQUIRE(p >= 1 && ds >= 1, "tile_grid_valid: read size p = %d and downsample factor ds = %d must be at least 1", p, ds);
    SQ_REQUIRE((long long)(n_col - 1) * p < (1ll << 31) && (long long)(n_row - 1) * p < (1ll << 31),
               "tile_grid_valid: grid of %d x %d tiles of %d pixels: a tile origin at or beyond 2^31", n_col, n_row, p);
    SQ_REQUIRE(pm >= 0 && pm <= SQ_TILE_GRID_MAX_WINDOW, "tile_grid_valid: window pm = %d, must be in 0..%d", pm, SQ_TILE_GRID_MAX_WINDOW);
    SQ_REQUIRE(iterations >= 0 && iterations <= SQ_TILE_GRID_MAX_ITERATIONS, "tile_grid_valid: iterations = %d, must be in 0..%d",
               iterations, SQ_TILE_GRID_MAX_ITERATIONS);
    SQ_REQUIRE(threshold == threshold, "tile_grid_valid: threshold is not a number");
    SQ_REQUIRE(mask_u8 && valid, "tile_grid_valid: null mask or valid pointer");
    SQ_REQUIRE(((uintptr_t)counts & 3) == 0 && ((uintptr_t)sizes & 3) == 0, "tile_grid_valid: misaligned counts or sizes (int32)");
    hipStream_t stream = (hipStream_t)stream_;
    TgArgs a;
    a.mask = mask_u8; a.valid = valid; a.counts = counts; a.sizes = sizes;
    a.mask_w = mask_w; a.mask_h = mask_h; a.n_col = n_col; a.n_row = n_row; a.p = p; a.ds = ds; a.pm = pm; a.iterations = iterations;
    a.tiles = n_col * n_row; a.threshold = threshold;
    if (pm <= 8) tg_launch_packed<8, uint32_t>(a, stream);
    else if (pm <= 16) tg_launch_packed<16, uint32_t>(a, stream);
    else if (pm <= 32) tg_launch_packed<32, uint32_t>(a, stream);
    else if (pm <= SQ_TILE_GRID_PACKED_MAX_WINDOW) tg_launch_packed<64, unsigned long long>(a, stream);
    else hipLaunchKernelGGL(tile_grid_wide_kernel, dim3((unsigned)a.tiles), dim3(TG_THREADS), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
