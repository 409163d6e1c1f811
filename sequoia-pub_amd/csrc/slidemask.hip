// Whole-slide tissue mask of patch generation on the device (include/sequoia_hip.h, "Slide mask"): get_mask_image of
// pre_processing/patch_gen_hdf5.py:25-38 on one uint8 image of any size, and the closing that extract_patches applies to it
// (:69-72: binary_dilation(iterations=3), then binary_erosion(iterations=3)).  The arithmetic is the per-tile filter's
// (patchfilter.h, shared with patchfilter.hip): single IEEE double operations in numpy's order, no fused multiply-add, so
// the four thresholds and every mask bit are the host's.  What differs is that an image spans many workgroups:
//   sweep 1   byte histograms of R, G, B; min and max of the saturation s                    (grid over chunks of 4096 pixels)
//   sweep 2   256-bin histogram of s between min and max with numpy's edges                   (the same grid)
//   otsu      one workgroup: three lanes walk the integer histograms, one lane the float one  (sequential, as np.cumsum is)
//   sweep 3   mask bits into a bit image in the workspace, ceil(w / 32) words per row; the raw count
//             (grid over pieces of rows: a piece starts at a multiple of 4096 pixels of its row, so the 64 lanes of a wave
//             hold 64 consecutive bits of one row and a ballot is two whole words: no atomics, nothing to clear)
//   closing   one workgroup per tile of 64 rows x 256 columns: the tile's bits and a halo of 2 k rows and one word of
//             columns in LDS, k steps of the cross, k steps of its erosion, popcounts, byte outputs (plain or transposed)
//   finish    the stats row
// Everything that crosses workgroups is order-independent: histogram and mask counts are integer atomic adds (a workgroup
// first counts in LDS copies chosen by the lane, as the per-tile kernel does: a blank slide sends every lane to one bin),
// min and max of s are integer atomics on the bit patterns of the non-negative doubles.  No floating-point sum crosses a
// workgroup, so two runs give the same bytes.  With h w <= 2^30 every count fits 32 bits and counts x centre sums stay
// below 2^53.  s is recomputed in every sweep (one double division per pixel) rather than stored: 8 bytes per pixel of
// traffic against 3.  With pixel_bytes = 4 (sq_slide_mask_px: the RGBA image a slide reader returns, the fourth byte ignored)
// the three sweeps load aligned dwords from global memory instead of staging 3-byte pixels; everything behind the load is the same.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"
#include "patchfilter.h"

#pragma clang fp contract(off)      // the whole file: no product may be fused into a following sum

namespace {

constexpr int SM_THREADS = 512, SM_WAVES = SM_THREADS / 64;
constexpr int SM_BYTE_COPIES = 4, SM_S_COPIES = 4;
constexpr int SM_MAX_BLOCKS = 2048;                    // sweeps: 256 CUs x 8; the chunks beyond are taken in strides
constexpr int SM_TILE_ROWS = 64, SM_TILE_COLS = 256;   // closing tile; patchgen.SLIDE_MASK_TILE mirrors it
constexpr int SM_TILE_WORDS = SM_TILE_COLS / 32;
constexpr int SM_CLOSE_THREADS = 256;
constexpr int SM_REGION_PITCH = SM_TILE_WORDS + 2;     // one halo word on either side: 32 >= 2 x SQ_SLIDE_MASK_MAX_ITERATIONS bits
constexpr int SM_REGION_ROWS = SM_TILE_ROWS + 4 * SQ_SLIDE_MASK_MAX_ITERATIONS;

// the head of the workspace, cleared on the stream by every call; the bit image follows at SM_HEAD_BYTES
struct SmHead {
    uint32_t hist_rgb[768];
    uint32_t hist_s[256];
    unsigned long long s_min_inv;    // ~bits(min s): grows by atomicMax from 0
    unsigned long long s_max_bits;   // bits(max s); s >= 0, so the bit patterns order like the values
    uint32_t count_raw, count_closed;
    int thr[3], pad;
    double thr_s;
};
constexpr size_t SM_HEAD_BYTES = 4352;

struct SmArgs {
    const uint8_t* src;
    SmHead* head;
    uint32_t* bits;          // [h][pitch]
    uint8_t* mask_raw;
    uint8_t* mask_closed;
    double* stats;
    int h, w, rgb_min, iterations, transpose;
    int pitch;               // 32-bit words per mask row
    int hw;
    int px;                  // bytes per pixel: 3, or 4 with the fourth ignored
};

__device__ __forceinline__ double sm_s_min(const SmHead* hd) { return __longlong_as_double((long long)~hd->s_min_inv); }
__device__ __forceinline__ double sm_s_max(const SmHead* hd) { return __longlong_as_double((long long)hd->s_max_bits); }

// f(r, g, b) for every pixel of the image: workgroup b takes the chunks b, b + gridDim.x, ...  3-byte pixels are staged in
// LDS, 4-byte pixels (the image 4-byte aligned) are loaded as dwords.
template <int PX, typename F>
__device__ __forceinline__ void sm_sweep(const SmArgs& a, uint8_t* stage, F&& f) {
    const uint8_t* const send = a.src + (size_t)a.hw * 3;
    const int chunks = (a.hw + PF_CHUNK_PX - 1) / PF_CHUNK_PX;
    if constexpr (PX == 4) {
        __syncthreads();                       // what the caller cleared is cleared before the first f
        for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
            const int base = c * PF_CHUNK_PX, npx = min(PF_CHUNK_PX, a.hw - base);
            pf_pixels4<SM_THREADS>(a.src + (size_t)base * 4, npx, [&](int, int r, int g, int b) { f(r, g, b); });
        }
        __syncthreads();
        return;
    }
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int base = c * PF_CHUNK_PX, npx = min(PF_CHUNK_PX, a.hw - base);
        const uint8_t* const s = stage + pf_stage<SM_THREADS>(a.src, send, a.src + (size_t)base * 3, npx, stage);
        for (int i = threadIdx.x; i < npx; i += SM_THREADS) f((int)s[3 * i], (int)s[3 * i + 1], (int)s[3 * i + 2]);
    }
    __syncthreads();
}

template <int PX>
__global__ __launch_bounds__(SM_THREADS) void slide_mask_sweep1_kernel(const SmArgs a) {
    __shared__ __align__(16) uint8_t stage[PX == 3 ? PF_STAGE_BYTES : 16];
    __shared__ uint32_t bh[SM_BYTE_COPIES * 768];
    __shared__ double wave_min[SM_WAVES], wave_max[SM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < SM_BYTE_COPIES * 768; i += SM_THREADS) bh[i] = 0u;
    double s_lo = 2.0, s_hi = 0.0;
    uint32_t* const my_bh = bh + (lane & (SM_BYTE_COPIES - 1)) * 768;
    sm_sweep<PX>(a, stage, [&](int r, int g, int b) {          // its first barrier orders the clearing before the adds
        atomicAdd(&my_bh[r], 1u);
        atomicAdd(&my_bh[256 + g], 1u);
        atomicAdd(&my_bh[512 + b], 1u);
        const double s = pf_saturation(r, g, b);
        s_lo = fmin(s_lo, s);
        s_hi = fmax(s_hi, s);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s_lo = fmin(s_lo, __shfl_xor(s_lo, o, 64));
        s_hi = fmax(s_hi, __shfl_xor(s_hi, o, 64));
    }
    if (lane == 0) wave_min[wave] = s_lo, wave_max[wave] = s_hi;
    for (int i = tid; i < 768; i += SM_THREADS) {
        uint32_t c = 0;
        for (int q = 0; q < SM_BYTE_COPIES; ++q) c += bh[q * 768 + i];
        if (c) atomicAdd(&a.head->hist_rgb[i], c);
    }
    __syncthreads();
    if (tid == 0) {
        double lo = wave_min[0], hi = wave_max[0];
        for (int i = 1; i < SM_WAVES; ++i) lo = fmin(lo, wave_min[i]), hi = fmax(hi, wave_max[i]);
        // every workgroup has at least one chunk (the grid is no larger than the chunk count), so lo <= 1 here
        atomicMax(&a.head->s_min_inv, ~(unsigned long long)__double_as_longlong(lo));
        atomicMax(&a.head->s_max_bits, (unsigned long long)__double_as_longlong(hi));
    }
}

template <int PX>
__global__ __launch_bounds__(SM_THREADS) void slide_mask_sweep2_kernel(const SmArgs a) {
#pragma clang fp contract(off)
    __shared__ __align__(16) uint8_t stage[PX == 3 ? PF_STAGE_BYTES : 16];
    __shared__ uint32_t shh[SM_S_COPIES * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const double s_min = sm_s_min(a.head), s_max = sm_s_max(a.head);
    if (!(s_min < s_max)) return;                          // constant s: the threshold is the value, no histogram (all workgroups alike)
    for (int i = tid; i < SM_S_COPIES * 256; i += SM_THREADS) shh[i] = 0u;
    const double step = (s_max - s_min) / 256.0;
    const double inv_step = 256.0 / (s_max - s_min);
    uint32_t* const my_sh = shh + (lane & (SM_S_COPIES - 1)) * 256;
    sm_sweep<PX>(a, stage, [&](int r, int g, int b) { atomicAdd(&my_sh[pf_bin(pf_saturation(r, g, b), s_min, s_max, step, inv_step)], 1u); });
    for (int i = tid; i < 256; i += SM_THREADS) {
        uint32_t c = 0;
        for (int q = 0; q < SM_S_COPIES; ++q) c += shh[q * 256 + i];
        if (c) atomicAdd(&a.head->hist_s[i], c);
    }
}

// one workgroup of four waves: lane 0 of waves 0..2 takes a channel, lane 0 of wave 3 the saturation
__global__ __launch_bounds__(256) void slide_mask_otsu_kernel(const SmArgs a) {
    __shared__ uint32_t cnt[1024];
    __shared__ double cs2[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 768; i += 256) cnt[i] = a.head->hist_rgb[i];
    cnt[768 + tid] = a.head->hist_s[tid];
    __syncthreads();
    if (lane != 0) return;
    if (wave < 3) {
        a.head->thr[wave] = pf_otsu_u8(cnt + wave * 256, a.hw);
    } else {
        const double s_min = sm_s_min(a.head), s_max = sm_s_max(a.head);
        a.head->thr_s = !(s_min < s_max) ? s_min : pf_otsu_s(cnt + 768, a.hw, s_min, s_max, cs2);
    }
}

// mask bits: a piece is up to 4096 pixels of one row from a multiple of 4096 on
template <int PX>
__global__ __launch_bounds__(SM_THREADS) void slide_mask_sweep3_kernel(const SmArgs a) {
    __shared__ __align__(16) uint8_t stage[PX == 3 ? PF_STAGE_BYTES : 16];
    __shared__ uint32_t wave_count[SM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* const send = a.src + (size_t)a.hw * 3;
    const double thr_s = a.head->thr_s;
    const int tr = a.head->thr[0], tg = a.head->thr[1], tb = a.head->thr[2], lowest = a.rgb_min;
    const int per_row = (a.w + PF_CHUNK_PX - 1) / PF_CHUNK_PX;
    const long long pieces = (long long)a.h * per_row;
    uint32_t count = 0;
    for (long long pc = blockIdx.x; pc < pieces; pc += gridDim.x) {
        const int y = (int)(pc / per_row), x0 = (int)(pc - (long long)y * per_row) * PF_CHUNK_PX;
        const int npx = min(PF_CHUNK_PX, a.w - x0);
        const uint8_t* s = stage;
        const uint32_t* const px = (const uint32_t*)(a.src + ((size_t)y * a.w + x0) * 4);      // PX == 4: the piece's dwords
        if constexpr (PX == 3) s += pf_stage<SM_THREADS>(a.src, send, a.src + ((size_t)y * a.w + x0) * 3, npx, stage);
        uint32_t* const row = a.bits + (size_t)y * a.pitch;
        for (int i0 = wave * 64; i0 < npx; i0 += SM_THREADS) {             // whole waves: the ballot needs every lane
            const int i = i0 + lane;
            bool on = false;
            if (i < npx) {
                int r, g, b;
                if constexpr (PX == 3) {
                    r = s[3 * i], g = s[3 * i + 1], b = s[3 * i + 2];
                } else {
                    const uint32_t v = px[i];
                    r = (int)(v & 255u), g = (int)((v >> 8) & 255u), b = (int)((v >> 16) & 255u);
                }
                const bool bright = r > tr && g > tg && b > tb;
                on = !bright && r > lowest && g > lowest && b > lowest && pf_saturation(r, g, b) > thr_s;
            }
            const unsigned long long m = __ballot(on);
            if (lane == 0) {
                const int word = (x0 + i0) >> 5;                           // x0 + i0 is a multiple of 64; word < pitch as i0 < npx
                row[word] = (uint32_t)m;
                if (word + 1 < a.pitch) row[word + 1] = (uint32_t)(m >> 32);
                count += (uint32_t)__popcll(m);
            }
        }
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        for (int i = 0; i < SM_WAVES; ++i) c += wave_count[i];
        if (c) atomicAdd(&a.head->count_raw, c);
    }
}

// scipy's binary_dilation(iterations=k) then binary_erosion(iterations=k) (the cross; both see zeros outside the image) of
// one tile.  The region in LDS is the tile plus 2 k rows above and below and one word left and right; what lies outside
// the image is zero and is cleared again after every step, what lies outside the region counts as zero too: that is wrong
// for positions inside the image, and the error moves inwards one position per step, 2 k in all -- the halo.
__global__ __launch_bounds__(SM_CLOSE_THREADS) void slide_mask_close_kernel(const SmArgs a) {
    __shared__ uint32_t buf[2][SM_REGION_ROWS * SM_REGION_PITCH];
    __shared__ uint32_t wave_count[SM_CLOSE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.iterations, halo = 2 * k;
    const int y0 = blockIdx.y * SM_TILE_ROWS, w0 = blockIdx.x * SM_TILE_WORDS;      // first row and first word of the tile
    const int rows = SM_TILE_ROWS + 2 * halo, words = rows * SM_REGION_PITCH;
    const uint32_t last_valid = (a.w & 31) ? (1u << (a.w & 31)) - 1u : 0xffffffffu;
    // the bits of region word (ry, j) that lie inside the image
    auto inside = [&](int ry, int j) -> uint32_t {
        const int gy = y0 - halo + ry, gw = w0 - 1 + j;
        if (gy < 0 || gy >= a.h || gw < 0 || gw >= a.pitch) return 0u;
        return gw == a.pitch - 1 ? last_valid : 0xffffffffu;
    };
    for (int i = tid; i < words; i += SM_CLOSE_THREADS) {
        const int ry = i / SM_REGION_PITCH, j = i - ry * SM_REGION_PITCH;
        const uint32_t ok = inside(ry, j);                    // sweep 3 leaves the bits beyond w zero; `ok` guards the address
        buf[0][i] = ok ? a.bits[(size_t)(y0 - halo + ry) * a.pitch + (w0 - 1 + j)] : 0u;
    }
    __syncthreads();
    const int th = min(SM_TILE_ROWS, a.h - y0), tw = min(SM_TILE_COLS, a.w - w0 * 32);   // the tile's extent inside the image
    // byte output of the tile from region buffer m
    auto emit = [&](const uint32_t* m, uint8_t* out) {
        if (!a.transpose) {
            for (int p = tid; p < th * SM_TILE_COLS; p += SM_CLOSE_THREADS) {
                const int ty = p / SM_TILE_COLS, tx = p - ty * SM_TILE_COLS;
                if (tx < tw) out[(size_t)(y0 + ty) * a.w + (w0 * 32 + tx)] = (uint8_t)((m[(halo + ty) * SM_REGION_PITCH + 1 + (tx >> 5)] >> (tx & 31)) & 1u);
            }
        } else {                                              // [w, h]: consecutive threads take consecutive rows of one column
            for (int p = tid; p < tw * SM_TILE_ROWS; p += SM_CLOSE_THREADS) {
                const int tx = p / SM_TILE_ROWS, ty = p - tx * SM_TILE_ROWS;
                if (ty < th) out[(size_t)(w0 * 32 + tx) * a.h + (y0 + ty)] = (uint8_t)((m[(halo + ty) * SM_REGION_PITCH + 1 + (tx >> 5)] >> (tx & 31)) & 1u);
            }
        }
    };
    if (a.mask_raw) emit(buf[0], a.mask_raw);
    for (int it = 0; it < 2 * k; ++it) {
        const uint32_t* const in = buf[it & 1];
        uint32_t* const out = buf[(it & 1) ^ 1];
        const bool dilate = it < k;
        for (int i = tid; i < words; i += SM_CLOSE_THREADS) {
            const int ry = i / SM_REGION_PITCH, j = i - ry * SM_REGION_PITCH;
            const uint32_t m = in[i];
            const uint32_t left = j > 0 ? in[i - 1] : 0u, right = j < SM_REGION_PITCH - 1 ? in[i + 1] : 0u;
            const uint32_t up = ry > 0 ? in[i - SM_REGION_PITCH] : 0u, down = ry < rows - 1 ? in[i + SM_REGION_PITCH] : 0u;
            const uint32_t from_left = (m << 1) | (left >> 31), from_right = (m >> 1) | (right << 31);
            const uint32_t o = dilate ? (m | from_left | from_right | up | down) : (m & from_left & from_right & up & down);
            out[i] = o & inside(ry, j);
        }
        __syncthreads();
    }
    const uint32_t* const fin = buf[0];                       // 2 k steps: an even number
    emit(fin, a.mask_closed);
    uint32_t count = 0;
    for (int i = tid; i < th * SM_TILE_WORDS; i += SM_CLOSE_THREADS) {
        const int ty = i / SM_TILE_WORDS, j = i - ty * SM_TILE_WORDS;
        count += __popc(fin[(halo + ty) * SM_REGION_PITCH + 1 + j]);       // the bits beyond the image are zero
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        for (int i = 0; i < SM_CLOSE_THREADS / 64; ++i) c += wave_count[i];
        if (c) atomicAdd(&a.head->count_closed, c);
    }
}

__global__ void slide_mask_finish_kernel(const SmArgs a) {
    if (threadIdx.x != 0) return;
    const SmHead* const hd = a.head;
    double* const row = a.stats;
    row[0] = (double)hd->thr[0], row[1] = (double)hd->thr[1], row[2] = (double)hd->thr[2], row[3] = hd->thr_s;
    row[4] = (double)hd->count_raw, row[5] = (double)hd->count_closed, row[6] = sm_s_min(hd), row[7] = sm_s_max(hd);
}

bool sm_shape_ok(const char* who, int h, int w) {
    if (h < 1 || h > SQ_SLIDE_MASK_MAX_DIM || w < 1 || w > SQ_SLIDE_MASK_MAX_DIM) {
        sq_set_error("%s: image of %d x %d: height and width must be in 1..%d", who, h, w, SQ_SLIDE_MASK_MAX_DIM);
        return false;
    }
    if ((long long)h * w > (1ll << 30)) {            // cannot happen while the extent bound is 2^15; stated, as the kernels rest on it
        sq_set_error("%s: image of %d x %d: more than 2^30 pixels (pixel counts are kept in 32 bits)", who, h, w);
        return false;
    }
    return true;
}

}  // namespace

static_assert(sizeof(SmHead) <= SM_HEAD_BYTES && SM_HEAD_BYTES % 256 == 0, "the bit image starts behind the head, aligned");
static_assert(SM_TILE_COLS % 32 == 0 && 2 * SQ_SLIDE_MASK_MAX_ITERATIONS <= 32, "one halo word covers 2 k columns");
static_assert(SQ_SLIDE_MASK_TILE_ROWS == SM_TILE_ROWS && SQ_SLIDE_MASK_TILE_COLS == SM_TILE_COLS, "the header states the tile");

extern "C" size_t sq_slide_mask_workspace_bytes(int h, int w) {
    if (!sm_shape_ok("slide_mask_workspace_bytes", h, w)) return 0;
    return SM_HEAD_BYTES + sq_align_up((size_t)h * ((w + 31) / 32) * sizeof(uint32_t), 256);
}

template <int PX>
static void sm_launch_sweeps(const SmArgs& a, unsigned sweep_grid, unsigned piece_grid, hipStream_t stream) {
    hipLaunchKernelGGL(slide_mask_sweep1_kernel<PX>, dim3(sweep_grid), dim3(SM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(slide_mask_sweep2_kernel<PX>, dim3(sweep_grid), dim3(SM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(slide_mask_otsu_kernel, dim3(1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(slide_mask_sweep3_kernel<PX>, dim3(piece_grid), dim3(SM_THREADS), 0, stream, a);
}

extern "C" int sq_slide_mask_px(const uint8_t* img_u8, int h, int w, int pixel_bytes, int rgb_min, int iterations, int transpose,
                                uint8_t* mask_raw, uint8_t* mask_closed, double* stats, void* workspace, size_t workspace_bytes,
                                sq_stream_t stream_) {
    if (!sm_shape_ok("slide_mask", h, w)) return SQ_ERR_ARG;
    SQ_REQUIRE(pixel_bytes == 3 || pixel_bytes == 4, "slide_mask: pixel_bytes = %d, must be 3 (RGB) or 4 (RGBA, the fourth byte ignored)",
               pixel_bytes);
    SQ_REQUIRE(img_u8 && mask_closed, "slide_mask: null image or mask_closed pointer");
    SQ_REQUIRE(pixel_bytes == 3 || ((uintptr_t)img_u8 & 3) == 0, "slide_mask: pixel_bytes = 4 takes a 4-byte aligned image");
    SQ_REQUIRE(iterations >= 0 && iterations <= SQ_SLIDE_MASK_MAX_ITERATIONS, "slide_mask: iterations = %d, must be in 0..%d", iterations,
               SQ_SLIDE_MASK_MAX_ITERATIONS);
    SQ_REQUIRE(((uintptr_t)stats & 7) == 0, "slide_mask: misaligned stats (doubles)");
    SQ_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "slide_mask: null or misaligned workspace (16 bytes)");
    const size_t need = sq_slide_mask_workspace_bytes(h, w);
    if (workspace_bytes < need) {
        sq_set_error("slide_mask: the workspace takes %zu bytes, %zu given", need, workspace_bytes);
        return SQ_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    SmArgs a;
    a.src = img_u8; a.head = (SmHead*)workspace; a.bits = (uint32_t*)((uint8_t*)workspace + SM_HEAD_BYTES);
    a.mask_raw = mask_raw; a.mask_closed = mask_closed; a.stats = stats;
    a.h = h; a.w = w; a.rgb_min = rgb_min; a.iterations = iterations; a.transpose = transpose != 0;
    a.pitch = (w + 31) / 32; a.hw = h * w; a.px = pixel_bytes;
    SQ_HIP_CHECK(hipMemsetAsync(workspace, 0, SM_HEAD_BYTES, stream));
    const int chunks = (a.hw + PF_CHUNK_PX - 1) / PF_CHUNK_PX;
    const unsigned sweep_grid = (unsigned)(chunks < SM_MAX_BLOCKS ? chunks : SM_MAX_BLOCKS);
    const long long pieces = (long long)h * ((w + PF_CHUNK_PX - 1) / PF_CHUNK_PX);
    const unsigned piece_grid = (unsigned)(pieces < SM_MAX_BLOCKS ? pieces : SM_MAX_BLOCKS);
    if (pixel_bytes == 3) sm_launch_sweeps<3>(a, sweep_grid, piece_grid, stream);
    else sm_launch_sweeps<4>(a, sweep_grid, piece_grid, stream);
    const dim3 tiles((unsigned)((w + SM_TILE_COLS - 1) / SM_TILE_COLS), (unsigned)((h + SM_TILE_ROWS - 1) / SM_TILE_ROWS));
    hipLaunchKernelGGL(slide_mask_close_kernel, tiles, dim3(SM_CLOSE_THREADS), 0, stream, a);
    if (stats) hipLaunchKernelGGL(slide_mask_finish_kernel, dim3(1), dim3(64), 0, stream, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_slide_mask(const uint8_t* img_u8, int h, int w, int rgb_min, int iterations, int transpose, uint8_t* mask_raw,
                             uint8_t* mask_closed, double* stats, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    return sq_slide_mask_px(img_u8, h, w, 3, rgb_min, iterations, transpose, mask_raw, mask_closed, stats, workspace, workspace_bytes,
                            stream_);
}
