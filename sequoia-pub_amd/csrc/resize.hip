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
    int n, h_in, w_in, h_out, w_out, ks_h, ks_v;
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
template <int KS>
__device__ __forceinline__ void rs_hrows(const uint8_t* __restrict__ s, int s_pitch, uint8_t* __restrict__ o, int o_pitch, int rows,
                                         const int (&k)[KS > 0 ? KS : 1], const int32_t* __restrict__ kx, int nx) {
#pragma unroll 2
    for (int r = 0; r < rows; ++r, s += s_pitch, o += o_pitch) {
        uint32_t c0 = 1u << (RS_PRECISION - 1), c1 = c0, c2 = c0;
        if constexpr (KS > 0) {
#pragma unroll
            for (int i = 0; i < KS; ++i) {     // taps beyond nx: coefficient 0 on staged or padding bytes
                c0 += rs_mul(k[i], s[3 * i]);
                c1 += rs_mul(k[i], s[3 * i + 1]);
                c2 += rs_mul(k[i], s[3 * i + 2]);
            }
        } else {
            for (int i = 0; i < nx; ++i) {
                const int kk = kx[i];
                c0 += rs_mul(kk, s[3 * i]);
                c1 += rs_mul(kk, s[3 * i + 1]);
                c2 += rs_mul(kk, s[3 * i + 2]);
            }
        }
        o[0] = (uint8_t)rs_clip8(c0);
        o[1] = (uint8_t)rs_clip8(c1);
        o[2] = (uint8_t)rs_clip8(c2);
    }
}

// KS > 0: ksize <= KS, coefficients in registers.  KS == 0: any ksize, coefficients read from the plan at every tap.
template <int KS>
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
    const size_t iw3 = (size_t)a.w_in * 3, ow3 = (size_t)a.w_out * 3;
    const uint8_t* const simg = a.src + (size_t)img * a.h_in * iw3;
    const uint8_t* const send = a.src + (size_t)a.n * a.h_in * iw3;

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
            rs_hrows<KS>(stage + skew + (size_t)xmin * 3, (int)iw3, inter + (size_t)(g0 - r0) * a.pitch + x * 3, a.pitch, g1 - g0, k, kx, nx);
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
bool rs_geometry(int h_in, int w_in, int h_out, int w_out, int filter, RsArgs* a, size_t* lds) {
    const size_t iw3 = (size_t)w_in * 3;
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

template <int KS>
int rs_launch(const RsArgs& a, size_t lds, hipStream_t st) {
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)resize_u8_kernel<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX));
        attr.done();
    }
    hipLaunchKernelGGL(resize_u8_kernel<KS>, dim3((unsigned)(a.n * a.bands)), dim3(RS_THREADS), lds, st, a);
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

extern "C" int sq_resize_u8(const uint8_t* src_u8, int n, int h_in, int w_in, uint8_t* dst_u8, int h_out, int w_out, int filter,
                            const int32_t* plan_dev, sq_stream_t stream_) {
    if (!rs_sizes_ok("resize_u8", h_in, w_in, h_out, w_out, filter)) return SQ_ERR_ARG;
    SQ_REQUIRE(src_u8 && dst_u8, "resize_u8: null image pointer");
    SQ_REQUIRE(plan_dev && ((uintptr_t)plan_dev & 3) == 0, "resize_u8: null or misaligned plan (upload what sq_resize_plan_init filled)");
    SQ_REQUIRE(n >= 1, "resize_u8: n = %d images", n);
    RsArgs a;
    a.src = src_u8; a.dst = dst_u8; a.plan = plan_dev;
    a.n = n; a.h_in = h_in; a.w_in = w_in; a.h_out = h_out; a.w_out = w_out;
    a.ks_h = rs_ksize(w_in, w_out, filter);
    a.ks_v = rs_ksize(h_in, h_out, filter);
    size_t lds = 0;
    if (!rs_geometry(h_in, w_in, h_out, w_out, filter, &a, &lds)) {
        sq_set_error("resize_u8: %d x %d -> %d x %d: one output row's band needs %zu bytes of LDS, a CU has %d", h_in, w_in, h_out, w_out,
                     lds, RS_LDS_MAX);
        return SQ_ERR_UNSUPPORTED;
    }
    SQ_REQUIRE((size_t)n * a.bands <= 0x7fffffffu, "resize_u8: %d images x %d bands exceed the grid", n, a.bands);
    const int ks = a.ks_h > a.ks_v ? a.ks_h : a.ks_v;
    hipStream_t st = (hipStream_t)stream_;
    if (ks <= 5) return rs_launch<5>(a, lds, st);       // bilinear down to 1/2, bicubic up
    if (ks <= 9) return rs_launch<9>(a, lds, st);       // bicubic down to 1/2, bilinear down to 1/4
    return rs_launch<0>(a, lds, st);
}
