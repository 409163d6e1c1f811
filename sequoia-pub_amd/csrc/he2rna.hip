// HE2RNA comparator (src/he2rna.py:42-106) -- the device side of forward_fixed_k after the per-tile MLP:
//   mask[b, n]   = max_c x[b, c, n] > 0                                              (he2rna.py:94-95)
//   s[b, g, n]   = scores[b, n, g] * mask[b, n]                                      (:96)
//   out_k[b, g]  = sum_{j<k} sorted_desc(s[b, g, :])[j] * mask[b, j] / sum_{j<k} mask[b, j]     (:97-98)
//   eval         = sum_k out_k / len(ks)                                             (:88-91)
// The 1x1 Conv1d layers of the MLP (:101-106) are sq_linear launches on the token-major tensor [B*N, C].
//
// A thread owns one (slide, gene) column of N <= 128 tile scores, kept in LDS as [n][thread] (conflict-free, reads
// coalesced over genes).  The descending sort is never materialised: the rank of every entry (entries that are larger,
// plus equal ones with a smaller tile index) says which position weight mask[b, rank] it meets and which of the top-k
// sums it belongs to.  O(N^2) compares per column -- 0.7 ms for 64 slides x 20 820 genes -- and the same ranks route
// the gradient in the backward kernel (d out / d s[n] = sum_{k > rank} scale * mask[b, rank] / cnt_k).
// Sums are accumulated in fp64 (the reference adds fp32 values in sorted order: equal within fp32 rounding).
#include "../../include/sequoia_hip.h"
#include "elementwise.h"
#include "he2rna.h"

namespace {

constexpr int HE_THREADS = 256;

__global__ __launch_bounds__(256) void he2rna_mask_kernel(const float* __restrict__ x, int rows, int C, float* __restrict__ mask) {
    // one wave per row: max over the C channels of a token-major row
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, x[(size_t)row * C + c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) mask[row] = m > 0.f ? 1.f : 0.f;
}

// GATHER: slide b is window b0 + blockIdx.y of a sliding-window map; its tile n is row gidx[b, n] of the per-tile score table and mask
// (a row outside [0, grows) is the zero padding: score 0, mask 0).  The values, the integer ranks, the fp64 sums over n in ascending
// order and the final mean are the batch kernel's, so a window's row is bit-identical to it on the materialised batch.  Two things
// differ in how the ranks are counted: HE_RANK_BLK positions against each LDS read, with the tie term only where it can apply
// (m < n: u >= v, which is (u > v) || (u == v) for every float, NaN included; m > n: u > v); and T = 128 threads per block, so the
// [N][T] value buffer (51 KB at N = 100) lets three blocks share a CU -- at T = 256 one block per CU leaves the LDS latency of the
// one-compare-per-read loop exposed.  Measured on a 50 000-tile slide at stride 1, G = 20 820: 8.7 s -> 2.5 s per slide, this kernel
// 2.4 s of it (LDS holds 100 values per column, so a CU runs 6 waves).
constexpr int HE_RANK_BLK = 8, HE_WIN_THREADS = 128;

template <bool BWD, bool GATHER = false, int T = HE_THREADS>
__global__ __launch_bounds__(T) void he2rna_topk_kernel(const float* __restrict__ scores, int lds_, const float* __restrict__ mask,
                                                        const HeKs ks, const float* __restrict__ gout, float* __restrict__ out,
                                                        int ldo, int N, int G, const int32_t* __restrict__ gidx = nullptr,
                                                        int grows = 0, int b0 = 0) {
    extern __shared__ float sval[];                  // [N][T]
    __shared__ float w[HE_MAX_N];                    // mask of the slide's tile positions
    __shared__ int32_t row[HE_MAX_N];                // GATHER: table row of each tile position, -1 = padding
    __shared__ double cnt[HE_MAX_KS];                // sum_{j<k} mask[b, j]
    const int b = b0 + blockIdx.y, g = blockIdx.x * T + threadIdx.x;
    const bool live = g < G;
    for (int n = threadIdx.x; n < N; n += T) {
        if constexpr (GATHER) {
            const int32_t r = gidx[(size_t)b * N + n];
            const bool ok = r >= 0 && r < grows;
            row[n] = ok ? r : -1;
            w[n] = ok ? mask[r] : 0.f;
        } else {
            w[n] = mask[(size_t)b * N + n];
        }
    }
    __syncthreads();
    if (threadIdx.x < ks.n) {
        double c = 0.0;
        for (int j = 0; j < ks.k[threadIdx.x]; ++j) c += (double)w[j];
        cnt[threadIdx.x] = c;
    }
    for (int n = 0; n < N; ++n) {
        if constexpr (GATHER) {
            const int32_t r = row[n];                // block-uniform: every lane reads the same table row, coalesced over genes
            sval[n * T + threadIdx.x] = live && r >= 0 ? scores[(size_t)r * lds_ + g] * w[n] : 0.f;
        } else {
            sval[n * T + threadIdx.x] = live ? scores[((size_t)b * N + n) * lds_ + g] * w[n] : 0.f;
        }
    }
    __syncthreads();
    double acc[HE_MAX_KS];
#pragma unroll
    for (int i = 0; i < HE_MAX_KS; ++i) acc[i] = 0.0;
    if constexpr (GATHER && !BWD) {
        for (int n0 = 0; n0 < N; n0 += HE_RANK_BLK) {
            float v[HE_RANK_BLK];
            int rk[HE_RANK_BLK];
#pragma unroll
            for (int j = 0; j < HE_RANK_BLK; ++j) {
                v[j] = n0 + j < N ? sval[(n0 + j) * T + threadIdx.x] : 0.f;
                rk[j] = 0;
            }
            int m = 0;
#pragma unroll 4
            for (; m < n0; ++m) {
                const float u = sval[m * T + threadIdx.x];
#pragma unroll
                for (int j = 0; j < HE_RANK_BLK; ++j) rk[j] += u >= v[j];
            }
            const int m1 = n0 + HE_RANK_BLK < N ? n0 + HE_RANK_BLK : N;
            for (; m < m1; ++m) {
                const float u = sval[m * T + threadIdx.x];
#pragma unroll
                for (int j = 0; j < HE_RANK_BLK; ++j) rk[j] += (u > v[j]) || (u == v[j] && m < n0 + j);
            }
#pragma unroll 4
            for (; m < N; ++m) {
                const float u = sval[m * T + threadIdx.x];
#pragma unroll
                for (int j = 0; j < HE_RANK_BLK; ++j) rk[j] += u > v[j];
            }
#pragma unroll
            for (int j = 0; j < HE_RANK_BLK; ++j) {
                if (n0 + j < N) {
                    const double wr = (double)w[rk[j]];
#pragma unroll
                    for (int i = 0; i < HE_MAX_KS; ++i)
                        if (i < ks.n && rk[j] < ks.k[i]) acc[i] += (double)v[j] * wr;
                }
            }
        }
    } else {
        const float go = BWD && live ? gout[(size_t)b * G + g] : 0.f;
        for (int n = 0; n < N; ++n) {
            const float v = sval[n * T + threadIdx.x];
            int r = 0;
            for (int m = 0; m < N; ++m) {
                const float u = sval[m * T + threadIdx.x];
                r += (u > v) || (u == v && m < n);
            }
            const double wr = (double)w[r];
            if constexpr (!BWD) {
#pragma unroll
                for (int i = 0; i < HE_MAX_KS; ++i)
                    if (i < ks.n && r < ks.k[i]) acc[i] += (double)v * wr;
            } else {
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < HE_MAX_KS; ++i)
                    if (i < ks.n && r < ks.k[i]) d += (double)ks.scale * wr / cnt[i];
                if (live) out[((size_t)b * N + n) * ldo + g] = (float)(d * (double)go) * w[n];
            }
        }
    }
    if constexpr (!BWD) {
        if (live) {
            float pred = 0.f;                        // pred += out_k / len(ks), in list order (he2rna.py:88-91)
            for (int i = 0; i < ks.n; ++i) pred += (float)(acc[i] / cnt[i]) * ks.scale;
            out[(size_t)b * ldo + g] = pred;
        }
    }
}

}  // namespace

extern "C" int sq_he2rna_tile_mask(const float* x_tokens, int n_rows, int n_channels, float* mask, sq_stream_t stream_) {
    SQ_REQUIRE(x_tokens && mask && n_rows >= 1 && n_channels >= 1, "he2rna_tile_mask: bad arguments");
    hipLaunchKernelGGL(he2rna_mask_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream_, x_tokens, n_rows, n_channels, mask);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_he2rna_topk_mean(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                                   float* out, int B, int N, int G, sq_stream_t stream_) {
    SQ_REQUIRE(scores && mask && out && B >= 1 && G >= 1 && ld_scores >= G, "he2rna_topk_mean: bad arguments");
    SQ_REQUIRE(N >= 1 && N <= HE_MAX_N, "he2rna_topk_mean: %d tiles per slide (1..%d)", N, HE_MAX_N);
    HeKs k;
    if (int e = he_fill_ks(ks, n_ks, scale, N, &k)) return e;
    const size_t lds = (size_t)N * HE_THREADS * sizeof(float);
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)he2rna_topk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, HE_MAX_N * HE_THREADS * 4));
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)he2rna_topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, HE_MAX_N * HE_THREADS * 4));
        attr.done();
    }
    hipLaunchKernelGGL(he2rna_topk_kernel<false>, dim3((G + HE_THREADS - 1) / HE_THREADS, B), dim3(HE_THREADS), lds, (hipStream_t)stream_,
                       scores, ld_scores, mask, k, (const float*)nullptr, out, G, N, G);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_he2rna_topk_mean_bwd(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                                       const float* grad_out, float* grad_scores, int ld_grad, int B, int N, int G, sq_stream_t stream_) {
    SQ_REQUIRE(scores && mask && grad_out && grad_scores && B >= 1 && G >= 1 && ld_scores >= G && ld_grad >= G, "he2rna_topk_mean_bwd: bad arguments");
    SQ_REQUIRE(N >= 1 && N <= HE_MAX_N, "he2rna_topk_mean_bwd: %d tiles per slide (1..%d)", N, HE_MAX_N);
    HeKs k;
    if (int e = he_fill_ks(ks, n_ks, scale, N, &k)) return e;
    const size_t lds = (size_t)N * HE_THREADS * sizeof(float);
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)he2rna_topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, HE_MAX_N * HE_THREADS * 4));
        attr.done();
    }
    hipLaunchKernelGGL(he2rna_topk_kernel<true>, dim3((G + HE_THREADS - 1) / HE_THREADS, B), dim3(HE_THREADS), lds, (hipStream_t)stream_,
                       scores, ld_scores, mask, k, grad_out, grad_scores, ld_grad, N, G);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_he2rna_window_topk_mean(const float* scores, int ld_scores, const float* mask, int gather_rows, const int32_t* gather_idx,
                                          const int32_t* ks, int n_ks, float scale, float* out, int n_windows, int N, int G,
                                          sq_stream_t stream_) {
    SQ_REQUIRE(scores && mask && gather_idx && out && n_windows >= 1 && G >= 1 && ld_scores >= G && gather_rows >= 1,
               "he2rna_window_topk_mean: bad arguments");
    SQ_REQUIRE(N >= 1 && N <= HE_MAX_N, "he2rna_window_topk_mean: %d tiles per window (1..%d)", N, HE_MAX_N);
    HeKs k;
    if (int e = he_fill_ks(ks, n_ks, scale, N, &k)) return e;
    const size_t lds = (size_t)N * HE_WIN_THREADS * sizeof(float);
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)he2rna_topk_kernel<false, true, HE_WIN_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         HE_MAX_N * HE_WIN_THREADS * 4));
        attr.done();
    }
    // gridDim.y is limited to 65535: windows go through in slabs (a window's row is the same arithmetic in any slab)
    for (int w0 = 0; w0 < n_windows; w0 += 65535) {
        const int nw = n_windows - w0 < 65535 ? n_windows - w0 : 65535;
        hipLaunchKernelGGL((he2rna_topk_kernel<false, true, HE_WIN_THREADS>), dim3((G + HE_WIN_THREADS - 1) / HE_WIN_THREADS, nw),
                           dim3(HE_WIN_THREADS), lds, (hipStream_t)stream_, scores, ld_scores, mask, k, (const float*)nullptr, out, G, N, G,
                           gather_idx, gather_rows, w0);
        SQ_LAUNCH_CHECK();
    }
    return SQ_OK;
}
