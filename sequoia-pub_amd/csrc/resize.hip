// Pillow-exact resize of uint8 NHWC patches (include/sequoia_hip.h, "Pillow-exact resize"): the resize the reference runs
// in front of its extractors -- transforms.Resize(224) on a PIL image (pre_processing/compute_features_hdf5.py:53-56,
// spatial_vis/visualize.py:226-230: BILINEAR) and patch.resize (pre_processing/patch_gen_hdf5.py:117: BICUBIC).
//
// The algorithm is Pillow's src/libImaging/Resample.c, restated:
//   precompute_coeffs      per axis: scale = in / out, filterscale = max(scale, 1), support = S filterscale, ksize =
//                          2 ceil(support) + 1; per output index the window [xmin, xmax) = [int(center - support + 0.5),
//                          int(center + support + 0.5)) clipped to the image, center = (xx + 0.5) scale; weights
//                          f((x + xmin - center + 0.5) (1 / filterscale)), summed in index order and divided by the sum
//   normalize_coeffs_8bpc  k = (int)(w 2^22 +- 0.5), truncating toward zero
//   ImagingResampleHorizontal_8bpc, ...Vertical_8bpc   acc = 2^21 + sum k[i] src[xmin + i] in int32; out = clip8(acc >> 22);
//                          the horizontal pass writes a uint8 image that the vertical pass reads
//   bilinear_filter, bicubic_filter (a = -0.5)
// The tables are double arithmetic without data: sq_resize_plan_init makes them on the host (no fused multiply-add: a
// contracted product rounds once where Pillow's build rounds twice), the caller uploads them once per shape.
//
// Kernel: a block takes one image and a band of R output rows.  It needs the input rows [r0, r1) that the band's vertical
// windows cover.  Those rows go through in groups: staged in LDS with 16-byte global loads (the rows of an image are one
// contiguous byte run), then the horizontal pass reads the staged bytes -- a thread owns one output column, its window
// start and coefficients in registers -- and writes the uint8 intermediate rows to LDS.  The vertical pass reads the
// intermediate rows a dword (four byte lanes) at a time, one wave per output row with the row's coefficients in scalar
// registers, and stores the output a dword per lane (256 contiguous bytes per wave instruction).  The intermediate image
// never goes to HBM.  No matrix instructions: the kernel moves bytes and does 24-bit integer multiply-adds.
// sq_resize_u8_gather puts a gather in front (image j is resized from src[index[j]]; an index out of range gives a zero image)
// and takes 3- or 4-byte source pixels (RGBA, the fourth byte ignored: a staged pixel is then one aligned LDS dword per tap);
// sq_resize_u8 is its call with 3-byte pixels and no index.  sq_pack_rgb_gather is the same gather without a resize.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"

#include <math.h>
#include <vector>

namespace {

constexpr int RS_THREADS = 256, RS_HEADER = 8, RS_PRECISION = 22;
constexpr int RS_LDS_MAX = 160 * 1024;         // LDS of a CU
constexpr int RS_LDS_WANT = 32 * 1024, RS_BAND_MAX = 16;      // measured, see rs_geometry
constexpr int RS_TAP_PAD = 32;                 // staged bytes a zero-coefficient tap may read past a group's last row (3 * 9 taps)

// ---- host: coefficient tables -------------------------------------------------------------------------------------------

double rs_filter(int filter, double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter == SQ_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double rs_support(int in, int out, int filter) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    return (filter == SQ_RESIZE_BILINEAR ? 1.0 : 2.0) * (scale < 1.0 ? 1.0 : scale);
}

int rs_ksize(int in, int out, int filter) { return in == out ? 1 : (int)ceil(rs_support(in, out, filter)) * 2 + 1; }

// bounds [out][2], coefs [out][ksize]; false when a coefficient leaves the 24-bit range the kernel multiplies in
bool rs_fill_axis(int in, int out, int filter, int32_t* bounds, int32_t* coefs) {
#pragma clang fp contract(off)
    const int ksize = rs_ksize(in, out, filter);
    if (in == out) {              // Pillow skips the pass; identity taps say the same
        for (int xx = 0; xx < out; ++xx) bounds[2 * xx] = xx, bounds[2 * xx + 1] = 1, coefs[xx] = 1 << RS_PRECISION;
        return true;
    }
    const double scale = (double)in / out, filterscale = scale < 1.0 ? 1.0 : scale, support = rs_support(in, out, filter);
    const double ss = 1.0 / filterscale;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = rs_filter(filter, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
        int32_t* k = coefs + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < n) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_PRECISION)) : (int)(0.5 + v * (1 << RS_PRECISION));
            if (k[x] >= (1 << 23) || k[x] <= -(1 << 23)) return false;
        }
    }
    return true;
}

bool rs_sizes_ok(const char* who, int h_in, int w_in, int h_out, int w_out, int filter) {
    if (filter != SQ_RESIZE_BILINEAR && filter != SQ_RESIZE_BICUBIC) {
        sq_set_error("%s: unknown filter %d (SQ_RESIZE_BILINEAR = 0, SQ_RESIZE_BICUBIC = 1)", who, filter);
        return false;
    }
    const int d[4] = {h_in, w_in, h_out, w_out};
    for (int v : d)
        if (v < 1 || v > SQ_RESIZE_MAX_DIM) {
            sq_set_error("%s: %d x %d -> %d x %d: every extent must be in 1..%d", who, h_in, w_in, h_out, w_out, SQ_RESIZE_MAX_DIM);
            return false;
        }
    return true;
}

// ---- device ---------------------------------------------------------------------------------------------------------------

struct RsArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* plan;
    const int32_t* index;   // [n] source image of every output image, or null for the identity
    int n, n_src;           // output images, source images
    int h_in, w_in, h_out, w_out, ks_h, ks_v;
    int band, bands;        // output rows per block, blocks per image
    int rows_cap;           // intermediate rows the LDS image holds
    int group;              // input rows staged at a time
    int stage_bytes, pitch; // LDS: staging buffer, bytes per intermediate row (multiple of 4)
};

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ uint32_t rs_clip8(uint32_t acc) { return (uint32_t)rs_clampi((int)acc >> RS_PRECISION, 0, 255); }
// k * v for |k| < 2^23 (checked when the plan is made) and a byte v: one full-rate v_mul_i32_i24.  A product is at most
// 255 * 2^22 < 2^30 wherever the normalised weight is <= 1 -- always for the bilinear filter; a bicubic window cut by the
// image edge can lift its largest weight to about 1.1 -- and the sum of a window stays inside int32 at these tap counts
// (sum |k| < 1.4 * 2^22).  The sums are kept in uint32 so that, like Pillow's int arithmetic in practice, they wrap.
__device__ __forceinline__ uint32_t rs_mul(int k, uint32_t v) { return (uint32_t)__mul24(k, (int)v); }

// Horizontal pass of one output column over `rows` staged rows: s = the column's first tap in the first row (s_pitch bytes per
// row), o = its three bytes in the first intermediate row.  The two LDS regions are separate __restrict__ arguments so that the
// reads of the next row may be issued before the byte stores of this one (both live in one LDS array, where the compiler has
// to assume they overlap); two rows per trip.
template <int KS, int PX>
__device__ __forceinline__ void rs_hrows(const uint8_t* __restrict__ s, int s_pitch, uint8_t* __restrict__ o, int o_pitch, int rows,
                                         const int (&k)[KS > 0 ? KS : 1], const int32_t* __restrict__ kx, int nx) {
#pragma unroll 2
    for (int r = 0; r < rows; ++r, s += s_pitch, o += o_pitch) {
        uint32_t c0 = 1u << (RS_PRECISION - 1), c1 = c0, c2 = c0;
        if constexpr (KS > 0) {
#pragma unroll
            for (int i = 0; i < KS; ++i) {     // taps beyond nx: coefficient 0 on staged or padding bytes
                if constexpr (PX == 4) {       // the source is 4-byte aligned, so a staged pixel is an aligned dword
                    const uint32_t v = *(const uint32_t*)(s + 4 * i);
                    c0 += rs_mul(k[i], v & 255u);
                    c1 += rs_mul(k[i], (v >> 8) & 255u);
                    c2 += rs_mul(k[i], (v >> 16) & 255u);
                } else {
                    c0 += rs_mul(k[i], s[3 * i]);
                    c1 += rs_mul(k[i], s[3 * i + 1]);
                    c2 += rs_mul(k[i], s[3 * i + 2]);
                }
            }
        } else {
            for (int i = 0; i < nx; ++i) {
                const int kk = kx[i];
                c0 += rs_mul(kk, s[PX * i]);
                c1 += rs_mul(kk, s[PX * i + 1]);
                c2 += rs_mul(kk, s[PX * i + 2]);
            }
        }
        o[0] = (uint8_t)rs_clip8(c0);
        o[1] = (uint8_t)rs_clip8(c1);
        o[2] = (uint8_t)rs_clip8(c2);
    }
}

// KS > 0: ksize <= KS, coefficients in registers.  KS == 0: any ksize, coefficients read from the plan at every tap.
// PX: bytes per source pixel, 3, or 4 with the fourth ignored; the output is always 3 bytes per pixel.
template <int KS, int PX>
__global__ __launch_bounds__(RS_THREADS) void resize_u8_kernel(const RsArgs a) {
    extern __shared__ __align__(16) uint8_t rs_lds[];
    uint8_t* const stage = rs_lds;
    uint8_t* const inter = rs_lds + a.stage_bytes;
    const int32_t* __restrict__ hb = a.plan + RS_HEADER;
    const int32_t* __restrict__ hc = hb + 2 * a.w_out;
    const int32_t* __restrict__ vb = hc + (size_t)a.w_out * a.ks_h;
    const int32_t* __restrict__ vc = vb + 2 * a.h_out;
    const int tid = threadIdx.x;
    const int img = blockIdx.x / a.bands, y0 = (blockIdx.x % a.bands) * a.band, y1 = min(y0 + a.band, a.h_out);
    // input rows of the band; every table value is clamped before it addresses anything
    const int r0 = rs_clampi(vb[2 * y0], 0, a.h_in - 1);
    const int r1 = rs_clampi(vb[2 * (y1 - 1)] + vb[2 * (y1 - 1) + 1], r0 + 1, min(a.h_in, r0 + a.rows_cap));
    const size_t iw3 = (size_t)a.w_in * PX, ow3 = (size_t)a.w_out * 3;      // bytes per input row, per output row
    // the source image: an index outside [0, n_src) is compared before any address is formed from it and gives a zero tile
    const int from = a.index ? a.index[img] : img;
    if (from < 0 || from >= a.n_src) {
        uint8_t* const z = a.dst + ((size_t)img * a.h_out + y0) * ow3;
        for (size_t i = tid; i < (size_t)(y1 - y0) * ow3; i += RS_THREADS) z[i] = 0;
        return;                                    // the whole block alike
    }
    const uint8_t* const simg = a.src + (size_t)from * a.h_in * iw3;
    const uint8_t* const send = a.src + (size_t)a.n_src * a.h_in * iw3;

    // ---- horizontal pass: input rows [r0, r1) -> inter[r - r0][w_out * 3]
    for (int g0 = r0; g0 < r1; g0 += a.group) {
        const int g1 = min(g0 + a.group, r1);
        const uint8_t* const p0 = simg + (size_t)g0 * iw3;
        const uint8_t* const lo = (const uint8_t*)((uintptr_t)p0 & ~(uintptr_t)15);
        const int skew = (int)(p0 - lo);
        const int chunks = (int)((simg + (size_t)g1 * iw3 - lo + 15) >> 4);
        __syncthreads();                           // the previous group has been read
        for (int c = tid; c < chunks; c += RS_THREADS) {
            const uint8_t* p = lo + (size_t)c * 16;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (p >= a.src && p + 16 <= send) {
                v = *(const u32x4*)p;
            } else {                               // the 16-byte lines at either end of the whole buffer
                for (int b = 0; b < 16; ++b)
                    if (p + b >= a.src && p + b < send) v[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
            }
            *(u32x4*)(stage + c * 16) = v;
        }
        __syncthreads();
        for (int xb = 0; xb < a.w_out; xb += RS_THREADS) {
            const int x = xb + tid;
            if (x >= a.w_out) continue;
            const int xmin = rs_clampi(hb[2 * x], 0, a.w_in - 1);
            const int nx = rs_clampi(hb[2 * x + 1], 0, min(a.ks_h, a.w_in - xmin));
            const int32_t* __restrict__ kx = hc + (size_t)x * a.ks_h;
            int k[KS > 0 ? KS : 1];
            if constexpr (KS > 0) {
#pragma unroll
                for (int i = 0; i < KS; ++i) k[i] = i < nx ? kx[i] : 0;
            }
            rs_hrows<KS, PX>(stage + skew + (size_t)xmin * PX, (int)iw3, inter + (size_t)(g0 - r0) * a.pitch + x * 3, a.pitch, g1 - g0, k, kx, nx);
        }
    }
    __syncthreads();

    // ---- vertical pass: one wave per output row, a dword of the row per lane
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int rows = r1 - r0, dwords = a.pitch >> 2;
    uint8_t* const dimg = a.dst + (size_t)img * a.h_out * ow3;
    const bool dword_stores = (((uintptr_t)dimg | ow3) & 3) == 0;      // every row of the image then starts on a dword
    for (int y = y0 + wave; y < y1; y += RS_THREADS / 64) {
        const int ymin = rs_clampi(vb[2 * y], r0, r1 - 1) - r0;
        const int ny = rs_clampi(vb[2 * y + 1], 0, min(a.ks_v, rows - ymin));
        const int32_t* __restrict__ ky = vc + (size_t)y * a.ks_v;
        int k[KS > 0 ? KS : 1];
        if constexpr (KS > 0) {
#pragma unroll
            for (int i = 0; i < KS; ++i) k[i] = i < ny ? ky[i] : 0;
        }
        const uint8_t* const col = inter + (size_t)ymin * a.pitch;
        for (int d = lane; d < dwords; d += 64) {
            uint32_t c0 = 1u << (RS_PRECISION - 1), c1 = c0, c2 = c0, c3 = c0;
            auto tap = [&](int kk, int i) {
                const uint32_t v = *(const uint32_t*)(col + (size_t)i * a.pitch + d * 4);
                c0 += rs_mul(kk, v & 255u);
                c1 += rs_mul(kk, (v >> 8) & 255u);
                c2 += rs_mul(kk, (v >> 16) & 255u);
                c3 += rs_mul(kk, v >> 24);
            };
            if constexpr (KS > 0) {
#pragma unroll
                for (int i = 0; i < KS; ++i)
                    if (i < ny) tap(k[i], i);           // wave-uniform
            } else {
                for (int i = 0; i < ny; ++i) tap(ky[i], i);
            }
            const uint32_t o = rs_clip8(c0) | rs_clip8(c1) << 8 | rs_clip8(c2) << 16 | rs_clip8(c3) << 24;
            uint8_t* q = dimg + (size_t)y * ow3 + d * 4;
            if (dword_stores) {
                *(uint32_t*)q = o;
            } else {
                for (int b = 0; b < 4; ++b)
                    if ((size_t)d * 4 + b < ow3) q[b] = (uint8_t)(o >> (8 * b));
            }
        }
    }
}

// Band height, staging group and LDS bytes for one shape.  The band is the tallest of 16, 8, ... 1 output rows whose LDS
// image stays at RS_LDS_WANT; failing that, the tallest that fits the CU at all.  A taller band repeats less of the horizontal
// pass (neighbouring bands share input rows) but leaves fewer blocks on a CU to hide each other's barriers and LDS latency,
// and the second matters more.  Measured, 1000 patches: 256 -> 224 bilinear 0.248 ms with 32 rows (33 KB, 4 blocks per CU),
// 0.184 ms with 16 (22 KB, 7 blocks); 512 -> 256 bicubic 0.985 ms with 16 rows (42 KB), 0.92 ms with 8 (26 KB), 1.02 ms with 4.
// A band of R rows covers at most (R - 1) scale + 2 support + 1 input rows (first window start to last window end), one
// more for the truncations.
bool rs_geometry(int h_in, int w_in, int h_out, int w_out, int filter, int px, RsArgs* a, size_t* lds) {
    const size_t iw3 = (size_t)w_in * px;
    a->pitch = (int)sq_align_up((size_t)w_out * 3, 4);
    a->group = (int)(8192 / iw3 < 1 ? 1 : 8192 / iw3 > 8 ? 8 : 8192 / iw3);
    a->stage_bytes = (int)sq_align_up((size_t)a->group * iw3 + 15 + 15 + RS_TAP_PAD, 16);
    const double scale = (double)h_in / h_out, support = rs_support(h_in, h_out, filter);
    size_t best = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int R = RS_BAND_MAX; R >= 1; R >>= 1) {
            const int band = R < h_out ? R : h_out;
            int rows = h_in == h_out ? band : (int)floor((band - 1) * scale + 2 * support + 1) + 1;
            if (rows > h_in) rows = h_in;
            const size_t need = a->stage_bytes + sq_align_up((size_t)rows * a->pitch, 16);
            best = need;
            if (need <= (size_t)(pass == 0 ? RS_LDS_WANT : RS_LDS_MAX)) {
                a->band = band;
                a->bands = (h_out + band - 1) / band;
                a->rows_cap = rows;
                *lds = need;
                return true;
            }
        }
    }
    *lds = best;
    return false;
}

template <int KS, int PX>
int rs_launch(const RsArgs& a, size_t lds, hipStream_t st) {
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)resize_u8_kernel<KS, PX>, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX));
        attr.done();
    }
    hipLaunchKernelGGL((resize_u8_kernel<KS, PX>), dim3((unsigned)(a.n * a.bands)), dim3(RS_THREADS), lds, st, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

}  // namespace

extern "C" size_t sq_resize_plan_bytes(int h_in, int w_in, int h_out, int w_out, int filter) {
    if (!rs_sizes_ok("resize_plan_bytes", h_in, w_in, h_out, w_out, filter)) return 0;
    const size_t words = RS_HEADER + (size_t)w_out * (2 + rs_ksize(w_in, w_out, filter)) + (size_t)h_out * (2 + rs_ksize(h_in, h_out, filter));
    return words * sizeof(int32_t);
}

extern "C" int sq_resize_plan_init(int h_in, int w_in, int h_out, int w_out, int filter, int32_t* plan, size_t plan_bytes) {
    if (!rs_sizes_ok("resize_plan_init", h_in, w_in, h_out, w_out, filter)) return SQ_ERR_ARG;
    SQ_REQUIRE(plan, "resize_plan_init: null plan");
    const size_t need = sq_resize_plan_bytes(h_in, w_in, h_out, w_out, filter);
    SQ_REQUIRE(plan_bytes >= need, "resize_plan_init: the plan takes %zu bytes, %zu given", need, plan_bytes);
    const int ks_h = rs_ksize(w_in, w_out, filter), ks_v = rs_ksize(h_in, h_out, filter);
    const int32_t head[RS_HEADER] = {h_in, w_in, h_out, w_out, filter, ks_h, ks_v, 0};
    for (int i = 0; i < RS_HEADER; ++i) plan[i] = head[i];
    int32_t* hb = plan + RS_HEADER;
    int32_t* hc = hb + 2 * w_out;
    int32_t* vb = hc + (size_t)w_out * ks_h;
    int32_t* vc = vb + 2 * h_out;
    SQ_REQUIRE(rs_fill_axis(w_in, w_out, filter, hb, hc) && rs_fill_axis(h_in, h_out, filter, vb, vc),
               "resize_plan_init: %d x %d -> %d x %d: a coefficient leaves the 24-bit range of the kernel's multiply", h_in, w_in, h_out, w_out);
    return SQ_OK;
}

namespace {

constexpr int PK_THREADS = 256;

struct PkArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* index;   // [m] or null for the identity
    int n_src, hw;          // source tiles, pixels per tile
    int quads, blocks;      // groups of four pixels per tile (the last may be short), blocks per tile
};

// dst[j] = the RGB bytes of src[index[j]]: a thread takes four pixels, 12 output bytes.  Where the tile's first byte is
// dword-aligned on either side the quad is loaded / stored as dwords (16 bytes at once where an RGBA tile starts on 16), else
// by the byte; the short last quad of a tile always goes by the byte.
template <int PX>
__global__ __launch_bounds__(PK_THREADS) void pack_rgb_kernel(const PkArgs a) {
    const int j = blockIdx.x / a.blocks, q = (blockIdx.x % a.blocks) * PK_THREADS + threadIdx.x;
    if (q >= a.quads) return;
    const int px0 = q * 4, npx = min(4, a.hw - px0);
    uint8_t* const o = a.dst + (size_t)j * a.hw * 3 + (size_t)px0 * 3;
    const bool out_dwords = npx == 4 && ((uintptr_t)o & 3) == 0;
    // the source tile: an index outside [0, n_src) is compared before any address is formed from it and gives a zero tile
    const int from = a.index ? a.index[j] : j;
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u;            // the quad's 12 output bytes, little-endian
    if (from >= 0 && from < a.n_src) {
        const uint8_t* const s = a.src + ((size_t)from * a.hw + px0) * PX;
        if (npx < 4) {
            for (int i = 0; i < npx; ++i)
                for (int c = 0; c < 3; ++c) o[3 * i + c] = s[PX * i + c];
            return;
        }
        if constexpr (PX == 4) {                   // s is 4-byte aligned: the tile base is, and a pixel is 4 bytes
            uint32_t v0, v1, v2, v3;
            if (((uintptr_t)s & 15) == 0) {
                const u32x4 v = *(const u32x4*)s;
                v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
            } else {
                const uint32_t* const p = (const uint32_t*)s;
                v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
            }
            v0 &= 0xffffffu, v1 &= 0xffffffu, v2 &= 0xffffffu, v3 &= 0xffffffu;
            w0 = v0 | v1 << 24, w1 = v1 >> 8 | v2 << 16, w2 = v2 >> 16 | v3 << 8;
        } else if (((uintptr_t)s & 3) == 0) {
            const uint32_t* const p = (const uint32_t*)s;
            w0 = p[0], w1 = p[1], w2 = p[2];
        } else {
            for (int b = 0; b < 4; ++b) {
                w0 |= (uint32_t)s[b] << (8 * b);
                w1 |= (uint32_t)s[4 + b] << (8 * b);
                w2 |= (uint32_t)s[8 + b] << (8 * b);
            }
        }
    } else if (npx < 4) {
        for (int i = 0; i < 3 * npx; ++i) o[i] = 0;
        return;
    }
    if (out_dwords) {
        uint32_t* const p = (uint32_t*)o;
        p[0] = w0, p[1] = w1, p[2] = w2;
    } else {
        for (int b = 0; b < 4; ++b) {
            o[b] = (uint8_t)(w0 >> (8 * b));
            o[4 + b] = (uint8_t)(w1 >> (8 * b));
            o[8 + b] = (uint8_t)(w2 >> (8 * b));
        }
    }
}

}  // namespace

extern "C" int sq_pack_rgb_gather(const uint8_t* src_u8, int n_src, int pixel_bytes, const int32_t* index, int m, int h, int w,
                                  uint8_t* dst_u8, sq_stream_t stream_) {
    SQ_REQUIRE(pixel_bytes == 3 || pixel_bytes == 4, "pack_rgb: pixel_bytes = %d, must be 3 (RGB) or 4 (RGBA, the fourth byte ignored)",
               pixel_bytes);
    SQ_REQUIRE(h >= 1 && h <= SQ_RESIZE_MAX_DIM && w >= 1 && w <= SQ_RESIZE_MAX_DIM, "pack_rgb: tiles of %d x %d: every extent must be in 1..%d",
               h, w, SQ_RESIZE_MAX_DIM);
    SQ_REQUIRE(m >= 0 && n_src >= 0, "pack_rgb: m = %d output tiles from n_src = %d", m, n_src);
    SQ_REQUIRE(index || m == n_src, "pack_rgb: a null index is the identity and takes m = n_src, got m = %d, n_src = %d", m, n_src);
    SQ_REQUIRE(((uintptr_t)index & 3) == 0, "pack_rgb: misaligned index (int32)");
    if (m == 0) return SQ_OK;
    SQ_REQUIRE(n_src >= 1, "pack_rgb: n_src = %d source tiles for m = %d output tiles", n_src, m);
    SQ_REQUIRE(src_u8 && dst_u8, "pack_rgb: null tile pointer");
    SQ_REQUIRE(pixel_bytes == 3 || ((uintptr_t)src_u8 & 3) == 0, "pack_rgb: pixel_bytes = 4 takes 4-byte aligned tiles");
    PkArgs a;
    a.src = src_u8; a.dst = dst_u8; a.index = index; a.n_src = n_src;
    a.hw = h * w;                                  // <= 2^28
    a.quads = (a.hw + 3) / 4;
    a.blocks = (a.quads + PK_THREADS - 1) / PK_THREADS;
    SQ_REQUIRE((size_t)m * a.blocks <= 0x7fffffffu, "pack_rgb: %d tiles x %d blocks exceed the grid", m, a.blocks);
    const dim3 grid((unsigned)((size_t)m * a.blocks));
    if (pixel_bytes == 3) hipLaunchKernelGGL(pack_rgb_kernel<3>, grid, dim3(PK_THREADS), 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL(pack_rgb_kernel<4>, grid, dim3(PK_THREADS), 0, (hipStream_t)stream_, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_resize_u8_gather(const uint8_t* src_u8, int n_src, int pixel_bytes, const int32_t* index, int m, int h_in, int w_in,
                                   uint8_t* dst_u8, int h_out, int w_out, int filter, const int32_t* plan_dev, sq_stream_t stream_) {
    if (!rs_sizes_ok("resize_u8", h_in, w_in, h_out, w_out, filter)) return SQ_ERR_ARG;
    SQ_REQUIRE(pixel_bytes == 3 || pixel_bytes == 4, "resize_u8: pixel_bytes = %d, must be 3 (RGB) or 4 (RGBA, the fourth byte ignored)",
               pixel_bytes);
    SQ_REQUIRE(m >= 0 && n_src >= 0, "resize_u8: m = %d output images from n_src = %d", m, n_src);
    SQ_REQUIRE(index || m == n_src, "resize_u8: a null index is the identity and takes m = n_src, got m = %d, n_src = %d", m, n_src);
    SQ_REQUIRE(((uintptr_t)index & 3) == 0, "resize_u8: misaligned index (int32)");
    SQ_REQUIRE(plan_dev && ((uintptr_t)plan_dev & 3) == 0, "resize_u8: null or misaligned plan (upload what sq_resize_plan_init filled)");
    if (m == 0) return SQ_OK;
    SQ_REQUIRE(n_src >= 1, "resize_u8: n_src = %d source images for m = %d output images", n_src, m);
    SQ_REQUIRE(src_u8 && dst_u8, "resize_u8: null image pointer");
    SQ_REQUIRE(pixel_bytes == 3 || ((uintptr_t)src_u8 & 3) == 0, "resize_u8: pixel_bytes = 4 takes 4-byte aligned images");
    RsArgs a;
    a.src = src_u8; a.dst = dst_u8; a.plan = plan_dev; a.index = index;
    a.n = m; a.n_src = n_src; a.h_in = h_in; a.w_in = w_in; a.h_out = h_out; a.w_out = w_out;
    a.ks_h = rs_ksize(w_in, w_out, filter);
    a.ks_v = rs_ksize(h_in, h_out, filter);
    size_t lds = 0;
    if (!rs_geometry(h_in, w_in, h_out, w_out, filter, pixel_bytes, &a, &lds)) {
        sq_set_error("resize_u8: %d x %d -> %d x %d: one output row's band needs %zu bytes of LDS, a CU has %d", h_in, w_in, h_out, w_out,
                     lds, RS_LDS_MAX);
        return SQ_ERR_UNSUPPORTED;
    }
    SQ_REQUIRE((size_t)m * a.bands <= 0x7fffffffu, "resize_u8: %d images x %d bands exceed the grid", m, a.bands);
    const int ks = a.ks_h > a.ks_v ? a.ks_h : a.ks_v;
    hipStream_t st = (hipStream_t)stream_;
    if (pixel_bytes == 3) {
        if (ks <= 5) return rs_launch<5, 3>(a, lds, st);       // bilinear down to 1/2, bicubic up
        if (ks <= 9) return rs_launch<9, 3>(a, lds, st);       // bicubic down to 1/2, bilinear down to 1/4
        return rs_launch<0, 3>(a, lds, st);
    }
    if (ks <= 5) return rs_launch<5, 4>(a, lds, st);
    if (ks <= 9) return rs_launch<9, 4>(a, lds, st);
    return rs_launch<0, 4>(a, lds, st);
}

extern "C" int sq_resize_u8(const uint8_t* src_u8, int n, int h_in, int w_in, uint8_t* dst_u8, int h_out, int w_out, int filter,
                            const int32_t* plan_dev, sq_stream_t stream_) {
    if (!rs_sizes_ok("resize_u8", h_in, w_in, h_out, w_out, filter)) return SQ_ERR_ARG;
    SQ_REQUIRE(src_u8 && dst_u8, "resize_u8: null image pointer");
    SQ_REQUIRE(n >= 1, "resize_u8: n = %d images", n);
    return sq_resize_u8_gather(src_u8, n, 3, nullptr, n, h_in, w_in, dst_u8, h_out, w_out, filter, plan_dev, stream_);
}
