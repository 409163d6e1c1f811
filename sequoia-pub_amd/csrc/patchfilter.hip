// Tissue and contrast filter of patch generation on the device (include/sequoia_hip.h, "Patch filter"): the per-tile test of
// pre_processing/patch_gen_hdf5.py:108-115 -- get_mask_image (:25-38: Otsu thresholds of R, G, B and of the HSV saturation),
// three binary dilations, a tissue count against background_threshold, and skimage's is_low_contrast -- with the arithmetic
// of sequoia-pub_amd/patchgen.py, which restates the scikit-image calls.  Every quantity except the luminance percentiles is
// a chain of single IEEE double operations in numpy's order, so the thresholds, masks and counts are the host's bit for bit
// as long as nothing is contracted into a fused multiply-add: the file is compiled under `#pragma clang fp contract(off)`
// (repeated in the functions that depend on it); the double division is hipcc's correctly rounded one.  The saturation, the
// histogram edges, the two Otsu walks and the staging of misaligned pixels live in patchfilter.h: the whole-slide mask
// (slidemask.hip) computes with the same functions.
//
// Kernel: one workgroup of 512 threads per tile, three sweeps over the tile's bytes.  A sweep stages 4096 pixels at a time
// in LDS with 16-byte global loads (tiles of an odd size start at every alignment: the loads are aligned down and the skew
// is applied when the staged bytes are read), then every thread takes pixels tid, tid + 512, ...  With pixel_bytes = 4
// (sq_patch_filter_px: RGBA as a slide reader returns it) a pixel is an aligned dword: a sweep loads the pixels straight from
// global memory, nothing is staged, and the same lambdas see the same r, g, b -- so every output is the 3-byte call's.
//   sweep 1   byte histograms of R, G, B; min and max of the saturation s; histogram of the upper 11 bits of the luminance
//             key 2125 R + 7154 G + 721 B (22 bits)
//             -> integer Otsu of the three channels (three lanes, one per channel: all sums are integers, one forward walk)
//             -> the upper key bits of the four order statistics the two percentiles interpolate between
//   sweep 2   256-bin histogram of s between min and max with numpy's edges; histograms of the lower 11 key bits under the
//             (at most four) selected upper parts
//             -> float Otsu on one lane: the two cumulative sums of counts * centre run sequentially, backward then
//                forward, as np.cumsum does -> thr_S; the four keys -> contrast ratio
//   sweep 3   mask bits (a row is ceil(w / 32) words) in LDS
//             -> three dilations with the cross on the bit rows, popcounts, optional byte masks
// s is recomputed in every sweep (three double divisions per pixel) rather than stored.  Histograms are LDS atomics on a few
// copies chosen by the lane index: a blank tile sends every lane to one bin, the copies cut that serialisation.  The four
// histograms of lower key bits have one copy each and combine equal keys within the wave before they add.
// The luminance is formed from the selected integer key, key / 2550000: numpy's BLAS product differs from any fixed-order
// sum in the last bit, so this one quantity is defined to 1e-12 and not to the bit (include/sequoia_hip.h).
#include "../../include/sequoia_hip.h"
#include "sq_common.h"
#include "patchfilter.h"

#pragma clang fp contract(off)      // the whole file: no product may be fused into a following sum

namespace {

constexpr int PF_THREADS = 512, PF_WAVES = PF_THREADS / 64;
constexpr int PF_KEY_LOW_BITS = 11, PF_KEY_BINS = 1 << PF_KEY_LOW_BITS;      // keys < 2 550 001 < 2^22
constexpr int PF_BYTE_COPIES = 4, PF_KEY_COPIES = 2, PF_S_COPIES = 4;
constexpr int PF_LDS_MAX = 160 * 1024;

struct PfArgs {
    const uint8_t* src;
    uint8_t* keep;
    double* rows;            // [n][8], never null (the caller's stats or the workspace)
    uint8_t* mask_raw;
    uint8_t* mask_dil;
    int n, h, w, rgb_min;
    double count_bound;      // fl(background_threshold * (double)(h w))
    double fraction;
    int pitch;               // 32-bit words per mask row
    int px;                  // bytes per pixel: 3, or 4 with the fourth ignored
};

struct alignas(16) PfShared {
    double cs2[256];         // float Otsu: backward cumulative sums
    double wave_min[PF_WAVES], wave_max[PF_WAVES];
    double s_min, s_max, thr_s, ratio;
    uint32_t wave_tot[PF_WAVES];
    int thr[3];
    uint32_t rank[4], rank_hi[4], rank_below[4], rank_slot[4], rank_key[4];
    uint32_t count_raw, count_dil, unused;
};

// np.percentile(.., q)'s virtual index n q + (1 - q) - 1 (method "linear"): lower rank and weight of the upper one
__device__ __forceinline__ void pf_rank(int n, double q, uint32_t* lower, double* gamma) {
#pragma clang fp contract(off)
    double vi = ((double)n * q + (1.0 + q * -1.0)) - 1.0;
    if (vi < 0.0) vi = 0.0;
    if (vi > (double)(n - 1)) vi = (double)(n - 1);
    const double fl = floor(vi);
    *lower = (uint32_t)fl;
    *gamma = vi - fl;
}

// numpy's _lerp
__device__ __forceinline__ double pf_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// exclusive prefix of one value per thread over the block; *total = the block's sum.  wave_tot: PF_WAVES words of LDS.
__device__ __forceinline__ uint32_t pf_block_exscan(uint32_t v, uint32_t* wave_tot, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();                           // the previous use of wave_tot has been read
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < PF_WAVES; ++i) {
        const uint32_t t = wave_tot[i];
        before += i < wave ? t : 0u;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// the bin of a 2048-bin histogram (`copies` copies, added) that holds the element of 0-based rank k, and the count below it
__device__ __forceinline__ void pf_select(const uint32_t* hist, int copies, uint32_t k, uint32_t* wave_tot, uint32_t* bin, uint32_t* below) {
    constexpr int PER = PF_KEY_BINS / PF_THREADS;
    uint32_t c[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = 0;
        for (int q = 0; q < copies; ++q) c[j] += hist[q * PF_KEY_BINS + threadIdx.x * PER + j];
        mine += c[j];
    }
    uint32_t total;
    uint32_t ex = pf_block_exscan(mine, wave_tot, &total);
    if (k >= total) k = total - 1;             // cannot happen: the ranks are below h w
    if (ex <= k && k < ex + mine) {            // exactly one thread
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (k < ex + c[j]) {
                *bin = threadIdx.x * PER + j;
                *below = ex;
                break;
            }
            ex += c[j];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void pf_zero(uint32_t* p, int words) {
    for (int i = threadIdx.x; i < words; i += PF_THREADS) p[i] = 0u;
}

// f(pixel index, r, g, b) for every pixel of the tile: 3-byte pixels staged through LDS, 4-byte pixels loaded as dwords
template <int PX, typename F>
__device__ __forceinline__ void pf_sweep(const PfArgs& a, int img, uint8_t* stage, F&& f) {
    const int tid = threadIdx.x, hw = a.h * a.w;
    if constexpr (PX == 4) {
        __syncthreads();                       // what the caller cleared is cleared before the first f
        pf_pixels4<PF_THREADS>(a.src + (size_t)img * hw * 4, hw, f);
        __syncthreads();
        return;
    }
    const uint8_t* const simg = a.src + (size_t)img * hw * 3;
    const uint8_t* const send = a.src + (size_t)a.n * hw * 3;
    for (int base = 0; base < hw; base += PF_CHUNK_PX) {
        const int npx = min(PF_CHUNK_PX, hw - base);
        const int skew = pf_stage<PF_THREADS>(a.src, send, simg + (size_t)base * 3, npx, stage);
        const uint8_t* const s = stage + skew;
        for (int i = tid; i < npx; i += PF_THREADS) f(base + i, (int)s[3 * i], (int)s[3 * i + 1], (int)s[3 * i + 2]);
    }
    __syncthreads();
}

template <int PX>
__global__ __launch_bounds__(PF_THREADS) void patch_filter_kernel(const PfArgs a) {
    extern __shared__ __align__(16) uint8_t pf_lds[];
    constexpr int STAGE = PX == 3 ? PF_STAGE_BYTES : 0;                      // dword pixels are not staged
    uint8_t* const stage = pf_lds;
    PfShared& sh = *(PfShared*)(pf_lds + STAGE);
    uint32_t* const hist = (uint32_t*)(pf_lds + STAGE + sizeof(PfShared));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.x, hw = a.h * a.w;

    // ---- sweep 1: byte histograms, range of s, upper key bits
    uint32_t* const bh = hist;                                              // [PF_BYTE_COPIES][3][256]
    uint32_t* const kh = hist + PF_BYTE_COPIES * 768;                       // [PF_KEY_COPIES][2048]
    pf_zero(hist, PF_BYTE_COPIES * 768 + PF_KEY_COPIES * PF_KEY_BINS);
    double s_lo = 2.0, s_hi = -1.0;
    {
        uint32_t* const my_bh = bh + (lane & (PF_BYTE_COPIES - 1)) * 768;
        uint32_t* const my_kh = kh + (lane & (PF_KEY_COPIES - 1)) * PF_KEY_BINS;
        pf_sweep<PX>(a, img, stage, [&](int, int r, int g, int b) {
            atomicAdd(&my_bh[r], 1u);
            atomicAdd(&my_bh[256 + g], 1u);
            atomicAdd(&my_bh[512 + b], 1u);
            atomicAdd(&my_kh[(2125 * r + 7154 * g + 721 * b) >> PF_KEY_LOW_BITS], 1u);
            const double s = pf_saturation(r, g, b);
            s_lo = fmin(s_lo, s);
            s_hi = fmax(s_hi, s);
        });
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s_lo = fmin(s_lo, __shfl_xor(s_lo, o, 64));
        s_hi = fmax(s_hi, __shfl_xor(s_hi, o, 64));
    }
    if (lane == 0) sh.wave_min[wave] = s_lo, sh.wave_max[wave] = s_hi;
    for (int i = tid; i < 768; i += PF_THREADS) {
        uint32_t c = 0;
        for (int q = 0; q < PF_BYTE_COPIES; ++q) c += bh[q * 768 + i];
        bh[i] = c;                             // copy 0 is read by this thread alone
    }
    __syncthreads();
    if (lane == 0 && wave < 3) sh.thr[wave] = pf_otsu_u8(bh + wave * 256, hw);
    if (tid == 3 * 64) {
        double lo = sh.wave_min[0], hi = sh.wave_max[0];
        for (int i = 1; i < PF_WAVES; ++i) lo = fmin(lo, sh.wave_min[i]), hi = fmax(hi, sh.wave_max[i]);
        sh.s_min = lo, sh.s_max = hi;
        double g0, g1;
        pf_rank(hw, 0.01, &sh.rank[0], &g0);
        pf_rank(hw, 0.99, &sh.rank[2], &g1);
        sh.rank[1] = min(sh.rank[0] + 1u, (uint32_t)hw - 1u);
        sh.rank[3] = min(sh.rank[2] + 1u, (uint32_t)hw - 1u);
    }
    __syncthreads();
    for (int r = 0; r < 4; ++r) pf_select(kh, PF_KEY_COPIES, sh.rank[r], sh.wave_tot, &sh.rank_hi[r], &sh.rank_below[r]);
    if (tid == 0) {                            // ranks under one upper part share a histogram of the lower bits
        for (int r = 0; r < 4; ++r) {
            uint32_t slot = r;
            for (int q = r - 1; q >= 0; --q)
                if (sh.rank_hi[q] == sh.rank_hi[r]) slot = q;
            sh.rank_slot[r] = slot;
        }
    }
    __syncthreads();

    // ---- sweep 2: histogram of s, lower key bits
    const double s_min = sh.s_min, s_max = sh.s_max;
    const bool s_const = !(s_min < s_max);
    uint32_t* const shh = hist;                                             // [PF_S_COPIES][256]
    uint32_t* const lh = hist + PF_S_COPIES * 256;                          // [4][2048] 
    uint32_t hi_of[4];
    bool own[4];
    for (int r = 0; r < 4; ++r) hi_of[r] = sh.rank_hi[r], own[r] = sh.rank_slot[r] == (uint32_t)r;
    __syncthreads();                           // every thread has read the upper parts before the histograms are cleared
    pf_zero(hist, PF_S_COPIES * 256 + 4 * PF_KEY_BINS);
    {
#pragma clang fp contract(off)
        const double step = (s_max - s_min) / 256.0;
        const double inv_step = s_const ? 0.0 : 256.0 / (s_max - s_min);
        uint32_t* const my_sh = shh + (lane & (PF_S_COPIES - 1)) * 256;
        pf_sweep<PX>(a, img, stage, [&](int, int r, int g, int b) {
            if (!s_const) atomicAdd(&my_sh[pf_bin(pf_saturation(r, g, b), s_min, s_max, step, inv_step)], 1u);
            const uint32_t key = 2125u * r + 7154u * g + 721u * b;
            const uint32_t hi = key >> PF_KEY_LOW_BITS, low = key & (PF_KEY_BINS - 1);
            // one copy per slot (four copies of 4 x 8 KiB would leave LDS for one workgroup per CU instead of three), so the
            // lanes of a wave that share the first hitting lane's key add once: a flat tile sends a whole wave to one bin
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!own[q]) continue;                                      // the same for the whole workgroup
                const bool hit = hi == hi_of[q];
                const unsigned long long hits = __ballot(hit);
                if (hits == 0ull) continue;                                 // the same for the wave's active lanes
                const int first = __ffsll(hits) - 1;
                const uint32_t first_low = (uint32_t)__shfl((int)low, first, 64);
                const unsigned long long same = __ballot(hit && low == first_low);
                if (lane == first) atomicAdd(&lh[q * PF_KEY_BINS + low], (uint32_t)__popcll(same));
                else if (hit && low != first_low) atomicAdd(&lh[q * PF_KEY_BINS + low], 1u);
            }
        });
    }
    for (int i = tid; i < 256; i += PF_THREADS) {
        uint32_t c = 0;
        for (int q = 0; q < PF_S_COPIES; ++q) c += shh[q * 256 + i];
        shh[i] = c;
    }
    __syncthreads();
    if (tid == 0) sh.thr_s = s_const ? s_min : pf_otsu_s(shh, hw, s_min, s_max, sh.cs2);
    for (int r = 0; r < 4; ++r)
        pf_select(lh + sh.rank_slot[r] * PF_KEY_BINS, 1, sh.rank[r] - sh.rank_below[r], sh.wave_tot, &sh.rank_key[r], &sh.unused);
    if (tid == 64) {
#pragma clang fp contract(off)
        double g[2];
        uint32_t dummy;
        pf_rank(hw, 0.01, &dummy, &g[0]);
        pf_rank(hw, 0.99, &dummy, &g[1]);
        double lum[4];
        for (int r = 0; r < 4; ++r) lum[r] = (double)((sh.rank_hi[r] << PF_KEY_LOW_BITS) | sh.rank_key[r]) / 2550000.0;
        sh.ratio = (pf_lerp(lum[2], lum[3], g[1]) - pf_lerp(lum[0], lum[1], g[0])) / 2.0;
        sh.count_raw = 0u, sh.count_dil = 0u;
    }
    __syncthreads();

    // ---- sweep 3: mask bits
    const int words = a.h * a.pitch;
    uint32_t* const m0 = hist;
    uint32_t* const m1 = hist + words;
    pf_zero(m0, words);
    {
        const double thr_s = sh.thr_s;
        const int tr = sh.thr[0], tg = sh.thr[1], tb = sh.thr[2], lowest = a.rgb_min;
        pf_sweep<PX>(a, img, stage, [&](int p, int r, int g, int b) {
            const bool bright = r > tr && g > tg && b > tb;
            if (!bright && r > lowest && g > lowest && b > lowest && pf_saturation(r, g, b) > thr_s) {
                const int y = p / a.w, x = p - y * a.w;
                atomicOr(&m0[y * a.pitch + (x >> 5)], 1u << (x & 31));
            }
        });
    }
    const uint32_t last_valid = (a.w & 31) ? (1u << (a.w & 31)) - 1u : 0xffffffffu;
    auto emit = [&](const uint32_t* m, uint8_t* out, uint32_t* counter) {
        uint32_t c = 0;
        for (int k = tid; k < words; k += PF_THREADS) c += __popc(m[k]);
        atomicAdd(counter, c);
        if (out) {
            uint8_t* const o = out + (size_t)img * hw;
            for (int p = tid; p < hw; p += PF_THREADS) {
                const int y = p / a.w, x = p - y * a.w;
                o[p] = (uint8_t)((m[y * a.pitch + (x >> 5)] >> (x & 31)) & 1u);
            }
        }
    };
    emit(m0, a.mask_raw, &sh.count_raw);
    // scipy's binary_dilation(iterations=3): the cross, zero outside the tile; m0 -> m1 -> m0 -> m1
    for (int it = 0; it < 3; ++it) {
        const uint32_t* const in = (it & 1) ? m1 : m0;
        uint32_t* const out = (it & 1) ? m0 : m1;
        for (int k = tid; k < words; k += PF_THREADS) {
            const int y = k / a.pitch, j = k - y * a.pitch;
            const uint32_t m = in[k];
            const uint32_t left = j > 0 ? in[k - 1] : 0u, right = j < a.pitch - 1 ? in[k + 1] : 0u;
            const uint32_t up = y > 0 ? in[k - a.pitch] : 0u, down = y < a.h - 1 ? in[k + a.pitch] : 0u;
            uint32_t o = m | (m << 1) | (left >> 31) | (m >> 1) | (right << 31) | up | down;
            if (j == a.pitch - 1) o &= last_valid;
            out[k] = o;
        }
        __syncthreads();
    }
    emit(m1, a.mask_dil, &sh.count_dil);
    __syncthreads();
    if (tid == 0) {
        double* const row = a.rows + (size_t)img * 8;
        const double dil = (double)sh.count_dil;
        row[0] = (double)sh.thr[0], row[1] = (double)sh.thr[1], row[2] = (double)sh.thr[2], row[3] = sh.thr_s;
        row[4] = (double)sh.count_raw, row[5] = dil, row[6] = sh.ratio, row[7] = 0.0;
        a.keep[img] = (uint8_t)(dil > a.count_bound && !(sh.ratio < a.fraction));
    }
}

bool pf_shape_ok(const char* who, int n, int h, int w) {
    if (n < 1) {
        sq_set_error("%s: n = %d tiles", who, n);
        return false;
    }
    if (h < SQ_PATCH_FILTER_MIN_DIM || h > SQ_PATCH_FILTER_MAX_DIM || w < SQ_PATCH_FILTER_MIN_DIM || w > SQ_PATCH_FILTER_MAX_DIM) {
        sq_set_error("%s: tiles of %d x %d: height and width must be in %d..%d (the tile's mask bits stay in LDS)", who, h, w,
                     SQ_PATCH_FILTER_MIN_DIM, SQ_PATCH_FILTER_MAX_DIM);
        return false;
    }
    return true;
}

// stage (3-byte pixels) | PfShared | the larger of the histograms (sweep 2: 4 KiB + 32 KiB) and the two bit masks
size_t pf_lds_bytes(int h, int w, int px) {
    const size_t hists = (size_t)(PF_S_COPIES * 256 + 4 * PF_KEY_BINS) * 4;
    const size_t masks = 2 * (size_t)h * ((w + 31) / 32) * 4;
    return (px == 3 ? PF_STAGE_BYTES : 0) + sizeof(PfShared) + (hists > masks ? hists : masks);
}

}  // namespace

static_assert(PF_STAGE_BYTES % 16 == 0 && sizeof(PfShared) % 16 == 0, "LDS regions stay 16-byte aligned");
static_assert((PF_BYTE_COPIES * 768 + PF_KEY_COPIES * PF_KEY_BINS) <= (PF_S_COPIES * 256 + 4 * PF_KEY_BINS), "sweep 1 fits sweep 2's region");
static_assert(PF_KEY_BINS % PF_THREADS == 0, "pf_select gives every thread the same number of bins");

extern "C" size_t sq_patch_filter_workspace_bytes(int n, int h, int w) {
    if (!pf_shape_ok("patch_filter_workspace_bytes", n, h, w)) return 0;
    return sq_align_up((size_t)n * 8 * sizeof(double), 256);
}

template <int PX>
static int pf_launch(const PfArgs& a, size_t lds, hipStream_t st) {
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)patch_filter_kernel<PX>, hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS_MAX));
        attr.done();
    }
    hipLaunchKernelGGL(patch_filter_kernel<PX>, dim3((unsigned)a.n), dim3(PF_THREADS), lds, st, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_patch_filter_px(const uint8_t* patches_u8, int n, int h, int w, int pixel_bytes, int rgb_min,
                                  double background_threshold, double contrast_fraction, uint8_t* keep, double* stats,
                                  uint8_t* mask_raw, uint8_t* mask_dilated, void* workspace, size_t workspace_bytes,
                                  sq_stream_t stream_) {
#pragma clang fp contract(off)
    if (!pf_shape_ok("patch_filter", n, h, w)) return SQ_ERR_ARG;
    SQ_REQUIRE(pixel_bytes == 3 || pixel_bytes == 4, "patch_filter: pixel_bytes = %d, must be 3 (RGB) or 4 (RGBA, the fourth byte ignored)",
               pixel_bytes);
    SQ_REQUIRE(patches_u8 && keep, "patch_filter: null patches or keep pointer");
    SQ_REQUIRE(pixel_bytes == 3 || ((uintptr_t)patches_u8 & 3) == 0, "patch_filter: pixel_bytes = 4 takes 4-byte aligned tiles");
    SQ_REQUIRE(((uintptr_t)stats & 7) == 0, "patch_filter: misaligned stats (doubles)");
    SQ_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "patch_filter: null or misaligned workspace (16 bytes)");
    const size_t need = sq_patch_filter_workspace_bytes(n, h, w);
    if (workspace_bytes < need) {
        sq_set_error("patch_filter: the workspace takes %zu bytes, %zu given", need, workspace_bytes);
        return SQ_ERR_WORKSPACE;
    }
    PfArgs a;
    a.src = patches_u8; a.keep = keep; a.rows = stats ? stats : (double*)workspace;
    a.mask_raw = mask_raw; a.mask_dil = mask_dilated;
    a.n = n; a.h = h; a.w = w; a.rgb_min = rgb_min;
    a.count_bound = background_threshold * (double)(h * w);
    a.fraction = contrast_fraction;
    a.pitch = (w + 31) / 32;
    a.px = pixel_bytes;
    const size_t lds = pf_lds_bytes(h, w, pixel_bytes);
    return pixel_bytes == 3 ? pf_launch<3>(a, lds, (hipStream_t)stream_) : pf_launch<4>(a, lds, (hipStream_t)stream_);
}

extern "C" int sq_patch_filter(const uint8_t* patches_u8, int n, int h, int w, int rgb_min, double background_threshold,
                               double contrast_fraction, uint8_t* keep, double* stats, uint8_t* mask_raw, uint8_t* mask_dilated,
                               void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    return sq_patch_filter_px(patches_u8, n, h, w, 3, rgb_min, background_threshold, contrast_fraction, keep, stats, mask_raw,
                              mask_dilated, workspace, workspace_bytes, stream_);
}
