// HE2RNA training step on the device (src/he2rna.py:108-127 around the model of :42-106): whole forward and backward passes
// over ONE flat padded parameter buffer, with three kernels of their own.
//   loss head : top-k mean over the tiles (he2rna.hip's rank / tie rule, first-k-positions mask, fp64 sums, 0/0 = NaN), the MSE
//               loss and the gradient of the scores in one launch.  A thread owns a (slide, gene) column as in he2rna.hip and ranks
//               it ONCE: the ranks stay in LDS as bytes (N <= 128) beside the values, pred[b, g] follows, and the gradient of entry
//               n is tab[rank[n]] * grad_scale * (pred - target) * mask[b, n] with tab[r] = sum_{k_i > r} scale * mask[b, r] / cnt_i
//               shared by the block.  128 threads: [N][128] floats + [N][128] bytes = 62.5 KB at N = 100, two blocks per CU.
//   dropout   : in place, u from Philox4x32-10 keyed by the seed on the counter (column / 4, row, layer, step): one call per four
//               elements, no stored mask, no dependence on the grid.
//   gate      : dX *= a > 0 ? 1 / (1 - p) : 0 on the saved post-dropout activation a (ReLU and dropout backward in one).
// The products are sq_linear / sq_linear_weight_grad (the fp32 MFMA engine) and sq_k_transpose.
#include "../../include/sequoia_hip.h"
#include "elementwise.h"
#include "gemm.h"
#include "he2rna.h"

namespace {

constexpr int LH_T = 128, LH_RANK_BLK = 8;
constexpr size_t HE_GEMM_WS_BYTES = 64ull << 20;      // split-K scratch of the products: what HE2RNA._workspace gives them

inline int up8(int n) { return (n + 7) / 8 * 8; }

__global__ __launch_bounds__(LH_T) void he2rna_loss_head_kernel(const float* __restrict__ scores, int lds_, const float* __restrict__ mask,
                                                                const HeKs ks, const float* __restrict__ target, float grad_scale,
                                                                float* __restrict__ pred, float* __restrict__ grad, int ldg, int N, int G,
                                                                double* __restrict__ partial) {
    extern __shared__ float sval[];                  // [N][T] masked scores, then [N][T] ranks as bytes
    __shared__ float w[HE_MAX_N];                    // mask of the slide's tile positions
    __shared__ double cnt[HE_MAX_KS];                // sum_{j<k} mask[b, j]
    __shared__ double tab[HE_MAX_N];                 // d pred / d (entry of rank r), before the entry's own mask
    __shared__ double red[LH_T / 64];
    uint8_t* srk = (uint8_t*)(sval + (size_t)N * LH_T);
    const int T = LH_T, b = blockIdx.y, g = blockIdx.x * T + threadIdx.x;
    const bool live = g < G;
    for (int n = threadIdx.x; n < N; n += T) w[n] = mask[(size_t)b * N + n];
    __syncthreads();
    if (threadIdx.x < ks.n) {
        double c = 0.0;
        for (int j = 0; j < ks.k[threadIdx.x]; ++j) c += (double)w[j];
        cnt[threadIdx.x] = c;
    }
    for (int n = 0; n < N; ++n) sval[n * T + threadIdx.x] = live ? scores[((size_t)b * N + n) * lds_ + g] * w[n] : 0.f;
    __syncthreads();
    for (int r = threadIdx.x; r < N; r += T) {       // the sum sq_he2rna_topk_mean_bwd makes per entry, once per rank
        const double wr = (double)w[r];
        double d = 0.0;
        for (int i = 0; i < ks.n; ++i)
            if (r < ks.k[i]) d += (double)ks.scale * wr / cnt[i];
        tab[r] = d;
    }
    double acc[HE_MAX_KS];
#pragma unroll
    for (int i = 0; i < HE_MAX_KS; ++i) acc[i] = 0.0;
    // ranks: entries that are larger, plus equal ones with a smaller tile index; LH_RANK_BLK positions against each LDS read, the tie
    // term only where it can apply (m < n: u >= v is (u > v) || (u == v) for every float, NaN included; m > n: u > v)
    for (int n0 = 0; n0 < N; n0 += LH_RANK_BLK) {
        float v[LH_RANK_BLK];
        int rk[LH_RANK_BLK];
#pragma unroll
        for (int j = 0; j < LH_RANK_BLK; ++j) {
            v[j] = n0 + j < N ? sval[(n0 + j) * T + threadIdx.x] : 0.f;
            rk[j] = 0;
        }
        int m = 0;
#pragma unroll 4
        for (; m < n0; ++m) {
            const float u = sval[m * T + threadIdx.x];
#pragma unroll
            for (int j = 0; j < LH_RANK_BLK; ++j) rk[j] += u >= v[j];
        }
        const int m1 = n0 + LH_RANK_BLK < N ? n0 + LH_RANK_BLK : N;
        for (; m < m1; ++m) {
            const float u = sval[m * T + threadIdx.x];
#pragma unroll
            for (int j = 0; j < LH_RANK_BLK; ++j) rk[j] += (u > v[j]) || (u == v[j] && m < n0 + j);
        }
#pragma unroll 4
        for (; m < N; ++m) {
            const float u = sval[m * T + threadIdx.x];
#pragma unroll
            for (int j = 0; j < LH_RANK_BLK; ++j) rk[j] += u > v[j];
        }
#pragma unroll
        for (int j = 0; j < LH_RANK_BLK; ++j) {
            if (n0 + j < N) {
                srk[(n0 + j) * T + threadIdx.x] = (uint8_t)rk[j];
                const double wr = (double)w[rk[j]];
#pragma unroll
                for (int i = 0; i < HE_MAX_KS; ++i)
                    if (i < ks.n && rk[j] < ks.k[i]) acc[i] += (double)v[j] * wr;
            }
        }
    }
    double sq = 0.0;
    float go = 0.f;
    if (live) {
        float p = 0.f;                               // pred += out_k / len(ks), in list order (he2rna.py:88-91)
        for (int i = 0; i < ks.n; ++i) p += (float)(acc[i] / cnt[i]) * ks.scale;
        pred[(size_t)b * G + g] = p;
        const float d = p - target[(size_t)b * G + g];
        go = grad_scale * d;
        sq = (double)d * (double)d;
    }
    __syncthreads();                                 // tab
    if (grad && live) {
        for (int n = 0; n < N; ++n) {
            const double d = tab[srk[n * T + threadIdx.x]];
            grad[((size_t)b * N + n) * ldg + g] = (float)(d * (double)go) * w[n];
        }
    }
    sq = wave_sum_f64(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < LH_T / 64; ++i) s += red[i];
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void he2rna_loss_final_kernel(const double* __restrict__ partial, int nblk, double inv_n, float* __restrict__ loss) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (float)((sh[0] + sh[1] + sh[2] + sh[3]) * inv_n);
}

// one wave per token row: the tile mask over all C channels (he2rna.py:94-95) and the last D channels (:102) as a zero-padded row
__global__ __launch_bounds__(256) void he2rna_input_kernel(const float* __restrict__ x, int rows, int C, int D, int ldd,
                                                           float* __restrict__ mask, float* __restrict__ a0) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) {
        const float v = x[(size_t)row * C + c];
        m = fmaxf(m, v);
        if (c >= C - D) a0[(size_t)row * ldd + (c - (C - D))] = v;
    }
    for (int c = D + lane; c < ldd; c += 64) a0[(size_t)row * ldd + c] = 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) mask[row] = m > 0.f ? 1.f : 0.f;
}

// columns [width, ld) of every row = 0: what a product with N = width leaves unwritten and the next one reads as K padding
__global__ __launch_bounds__(256) void he2rna_pad_zero_kernel(float* __restrict__ a, int rows, int width, int ld) {
    const int pad = ld - width;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)rows * pad) a[(i / pad) * ld + width + (int)(i % pad)] = 0.f;
}

struct Philox { uint32_t v[4]; };
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

// thread = four consecutive columns of a row.  VEC: rows are 16-byte aligned and the thread's four columns lie inside the width.
template <bool GATE>
__global__ __launch_bounds__(256) void he2rna_dropout_kernel(float* __restrict__ y, int ldy, const float* __restrict__ a, int lda, int rows,
                                                             int width, int vec, float p, float inv_keep, uint32_t k0, uint32_t k1,
                                                             uint32_t layer, uint32_t step) {
    const int ngrp = (width + 3) / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * ngrp) return;
    const int row = (int)(i / ngrp), grp = (int)(i % ngrp), c = grp * 4;
    float f[4];
    if constexpr (GATE) {
        if (vec && c + 4 <= width) {
            const float4 av = *(const float4*)(a + (size_t)row * lda + c);
            f[0] = av.x; f[1] = av.y; f[2] = av.z; f[3] = av.w;
        } else {
            for (int j = 0; j < 4; ++j) f[j] = c + j < width ? a[(size_t)row * lda + c + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = f[j] > 0.f ? inv_keep : 0.f;
    } else {
        const Philox r = philox4x32_10((uint32_t)grp, (uint32_t)row, layer, step, k0, k1);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = (float)(r.v[j] >> 8) * 0x1p-24f >= p ? inv_keep : 0.f;      // u in [0, 1), kept when u >= p
    }
    float* yr = y + (size_t)row * ldy + c;
    if (vec && c + 4 <= width) {
        float4 v = *(float4*)yr;
        v.x = f[0] != 0.f ? v.x * f[0] : 0.f; v.y = f[1] != 0.f ? v.y * f[1] : 0.f;
        v.z = f[2] != 0.f ? v.z * f[2] : 0.f; v.w = f[3] != 0.f ? v.w * f[3] : 0.f;
        *(float4*)yr = v;
    } else {
        for (int j = 0; j < 4 && c + j < width; ++j) yr[j] = f[j] != 0.f ? yr[j] * f[j] : 0.f;
    }
}

int launch_elementwise(bool gate, float* y, int ldy, const float* a, int lda, int rows, int width, float p, long long seed, int layer,
                       long long step, hipStream_t st) {
    const bool vec = ldy % 4 == 0 && ((uintptr_t)y & 15) == 0 && (!gate || (lda % 4 == 0 && ((uintptr_t)a & 15) == 0));
    const size_t n = (size_t)rows * ((width + 3) / 4);
    const float inv_keep = 1.0f / (1.0f - p);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (gate)
        hipLaunchKernelGGL(he2rna_dropout_kernel<true>, grid, dim3(256), 0, st, y, ldy, a, lda, rows, width, (int)vec, p, inv_keep, 0u, 0u, 0u, 0u);
    else
        hipLaunchKernelGGL(he2rna_dropout_kernel<false>, grid, dim3(256), 0, st, y, ldy, a, lda, rows, width, (int)vec, p, inv_keep,
                           (uint32_t)(unsigned long long)seed, (uint32_t)((unsigned long long)seed >> 32), (uint32_t)layer, (uint32_t)step);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

int pad_zero(float* a, int rows, int width, int ld, hipStream_t st) {
    if (ld == width) return SQ_OK;
    const size_t n = (size_t)rows * (ld - width);
    hipLaunchKernelGGL(he2rna_pad_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, rows, width, ld);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

// The workspace of a step, in floats from its start (every piece 256-byte aligned): what the forward pass saves, the backward reads.
struct HePlan {
    int L, M, ld[SQ_HE2RNA_MAX_LAYERS + 1];
    int64_t w_off[SQ_HE2RNA_MAX_LAYERS], b_off[SQ_HE2RNA_MAX_LAYERS], n_params;
    size_t mask, act[SQ_HE2RNA_MAX_LAYERS + 1], gscores, dx[2], wt, head, gemm, bytes;
};

int he_param_layout(const int32_t* dims, int n_layers, int64_t* w_off, int64_t* b_off, int64_t* total) {
    SQ_REQUIRE(dims && n_layers >= 1 && n_layers <= SQ_HE2RNA_MAX_LAYERS, "he2rna_param_layout: %d layers (1..%d)", n_layers, SQ_HE2RNA_MAX_LAYERS);
    int64_t off = 0;
    for (int i = 0; i <= n_layers; ++i) SQ_REQUIRE(dims[i] >= 1, "he2rna_param_layout: width %d of layer %d", dims[i], i);
    for (int i = 0; i < n_layers; ++i) {
        if (w_off) w_off[i] = off;
        off += (int64_t)dims[i + 1] * up8(dims[i]);        // [n_out, round_up(n_in, 8)]: a multiple of 8 floats
        if (b_off) b_off[i] = off;
        off += (dims[i + 1] + 3) / 4 * 4;                  // the next tensor starts on a 16-byte boundary
    }
    if (total) *total = off;
    return SQ_OK;
}

int he_plan(const char* name, const int32_t* dims, int n_layers, int B, int N, HePlan* p) {
    if (int e = he_param_layout(dims, n_layers, p->w_off, p->b_off, &p->n_params)) return e;
    SQ_REQUIRE(B >= 1 && B <= 65535, "%s: batch = %d slides (1..65535)", name, B);
    SQ_REQUIRE(N >= 1 && N <= HE_MAX_N, "%s: %d tiles per slide (1..%d)", name, N, HE_MAX_N);
    p->L = n_layers;
    p->M = B * N;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t at = off; off += sq_align_up(floats * 4, 256) / 4; return at; };
    int hid = 0;
    size_t wt = 0;
    for (int i = 0; i <= n_layers; ++i) {
        p->ld[i] = up8(dims[i]);
        SQ_REQUIRE((size_t)p->M * p->ld[i] * 4 < (1ull << 31), "%s: a [%d, %d] fp32 activation does not fit a 2 GiB buffer descriptor", name, p->M, p->ld[i]);
    }
    for (int i = 1; i < n_layers; ++i) {             // hidden layers: the widest dX table, the largest transposed weight
        hid = p->ld[i] > hid ? p->ld[i] : hid;
        const size_t t = (size_t)p->ld[i] * p->ld[i + 1];
        wt = t > wt ? t : wt;
    }
    p->mask = take(p->M);
    for (int i = 0; i <= n_layers; ++i) p->act[i] = take((size_t)p->M * p->ld[i]);
    p->gscores = take((size_t)p->M * p->ld[n_layers]);
    p->dx[0] = take((size_t)p->M * hid);
    p->dx[1] = take((size_t)p->M * hid);
    p->wt = take(wt);
    p->head = take(sq_he2rna_loss_head_workspace_bytes(B, dims[n_layers]) / 4);
    p->gemm = take(HE_GEMM_WS_BYTES / 4);
    p->bytes = off * 4;
    return SQ_OK;
}

}  // namespace

extern "C" int sq_he2rna_param_layout(const int32_t* dims, int n_layers, int64_t* w_off, int64_t* b_off, int64_t* total) {
    return he_param_layout(dims, n_layers, w_off, b_off, total);
}

extern "C" size_t sq_he2rna_loss_head_workspace_bytes(int B, int G) {
    if (B < 1 || G < 1) return 0;
    return (size_t)B * ((G + LH_T - 1) / LH_T) * sizeof(double);
}

extern "C" int sq_he2rna_loss_head(const float* scores, int ld_scores, const float* mask, const int32_t* ks, int n_ks, float scale,
                                   const float* target, float grad_scale, float* pred, float* loss_out, float* grad_scores, int ld_grad,
                                   int B, int N, int G, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE(scores && mask && target && pred && loss_out && workspace && B >= 1 && B <= 65535 && G >= 1 && ld_scores >= G &&
               (!grad_scores || ld_grad >= G), "he2rna_loss_head: bad arguments");
    SQ_REQUIRE(N >= 1 && N <= HE_MAX_N, "he2rna_loss_head: %d tiles per slide (1..%d)", N, HE_MAX_N);
    SQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "he2rna_loss_head: the workspace must be 8-byte aligned");
    SQ_REQUIRE_WORKSPACE("he2rna_loss_head", workspace_bytes, sq_he2rna_loss_head_workspace_bytes(B, G));
    HeKs k;
    if (int e = he_fill_ks(ks, n_ks, scale, N, &k)) return e;
    static SqDevOnce attr;       // hipFuncSetAttribute is per device
    if (attr.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)he2rna_loss_head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HE_MAX_N * LH_T * 5));
        attr.done();
    }
    hipStream_t st = (hipStream_t)stream_;
    const int gx = (G + LH_T - 1) / LH_T;
    hipLaunchKernelGGL(he2rna_loss_head_kernel, dim3(gx, B), dim3(LH_T), (size_t)N * LH_T * 5, st, scores, ld_scores, mask, k, target,
                       grad_scale, pred, grad_scores, ld_grad, N, G, (double*)workspace);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(he2rna_loss_final_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, gx * B, 1.0 / ((double)B * G), loss_out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_he2rna_dropout(float* act, int ld, int rows, int width, float p, long long seed, long long step, int layer,
                                 sq_stream_t stream_) {
    SQ_REQUIRE(act && rows >= 1 && width >= 1 && ld >= width, "he2rna_dropout: bad arguments");
    SQ_REQUIRE(p >= 0.f && p < 1.f, "he2rna_dropout: p = %g must be in [0, 1) (p >= 1 drops every unit)", (double)p);
    SQ_REQUIRE(step >= 0 && step <= 0xFFFFFFFFll && layer >= 0, "he2rna_dropout: step index %lld must be in 0..2^32-1", step);
    if (p == 0.f) return SQ_OK;
    return launch_elementwise(false, act, ld, nullptr, 0, rows, width, p, seed, layer, step, (hipStream_t)stream_);
}

extern "C" int sq_he2rna_dropout_gate(float* grad, int ld_grad, const float* act, int ld_act, int rows, int width, float p,
                                      sq_stream_t stream_) {
    SQ_REQUIRE(grad && act && rows >= 1 && width >= 1 && ld_grad >= width && ld_act >= width, "he2rna_dropout_gate: bad arguments");
    SQ_REQUIRE(p >= 0.f && p < 1.f, "he2rna_dropout_gate: p = %g must be in [0, 1) (p >= 1 drops every unit)", (double)p);
    return launch_elementwise(true, grad, ld_grad, act, ld_act, rows, width, p, 0, 0, 0, (hipStream_t)stream_);
}

extern "C" size_t sq_he2rna_train_workspace_bytes(const int32_t* dims, int n_layers, int B, int N, int64_t* act_offsets) {
    HePlan p;
    if (he_plan("he2rna_train_workspace_bytes", dims, n_layers, B, N, &p)) return 0;
    if (act_offsets)
        for (int i = 0; i <= n_layers; ++i) act_offsets[i] = (int64_t)p.act[i];
    return p.bytes;
}

extern "C" int sq_he2rna_train_forward(const float* x, int B, int N, int C, const int32_t* dims, int n_layers, const float* params,
                                       const int32_t* ks, int n_ks, float scale, float p_drop, long long seed, long long step,
                                       const float* target, float grad_scale, float* pred, float* loss_out, void* workspace,
                                       size_t workspace_bytes, sq_stream_t stream) {
    HePlan P;
    if (int e = he_plan("he2rna_train_forward", dims, n_layers, B, N, &P)) return e;
    SQ_REQUIRE(x && params && target && pred && loss_out && workspace, "he2rna_train_forward: null pointer");
    SQ_REQUIRE(C >= dims[0], "he2rna_train_forward: %d channels, the model reads the last %d", C, dims[0]);
    SQ_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "he2rna_train_forward: dropout p = %g must be in [0, 1) (p >= 1 drops every unit)", (double)p_drop);
    SQ_REQUIRE(step >= 0 && step <= 0xFFFFFFFFll, "he2rna_train_forward: step index %lld must be in 0..2^32-1", step);
    SQ_REQUIRE((((uintptr_t)workspace | (uintptr_t)params) & 15) == 0, "he2rna_train_forward: params and workspace must be 16-byte aligned");
    SQ_REQUIRE_WORKSPACE("he2rna_train_forward", workspace_bytes, P.bytes);
    HeKs kchk;
    if (int e = he_fill_ks(ks, n_ks, scale, N, &kchk)) return e;      // refuse before anything is launched
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int M = P.M, L = P.L, G = dims[L];
    hipLaunchKernelGGL(he2rna_input_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, M, C, dims[0], P.ld[0], ws + P.mask, ws + P.act[0]);
    SQ_LAUNCH_CHECK();
    for (int i = 0; i < L; ++i) {
        const bool last = i + 1 == L;
        float* out = ws + P.act[i + 1];
        if (int e = sq_linear(SQ_F32, ws + P.act[i], P.ld[i], params + P.w_off[i], P.ld[i], params + P.b_off[i], nullptr, 0, SQ_F32,
                              last ? SQ_ACT_NONE : SQ_ACT_RELU, out, SQ_F32, P.ld[i + 1], M, dims[i + 1], P.ld[i], ws + P.gemm,
                              HE_GEMM_WS_BYTES, stream)) return e;
        if (last) break;
        if (int e = pad_zero(out, M, dims[i + 1], P.ld[i + 1], st)) return e;
        if (p_drop > 0.f)
            if (int e = launch_elementwise(false, out, P.ld[i + 1], nullptr, 0, M, dims[i + 1], p_drop, seed, i, step, st)) return e;
    }
    if (int e = pad_zero(ws + P.gscores, M, G, P.ld[L], st)) return e;       // the K padding of the first dX product
    return sq_he2rna_loss_head(ws + P.act[L], P.ld[L], ws + P.mask, ks, n_ks, scale, target, grad_scale, pred, loss_out, ws + P.gscores,
                               P.ld[L], B, N, G, ws + P.head, sq_he2rna_loss_head_workspace_bytes(B, G), stream);
}

extern "C" int sq_he2rna_train_backward(int B, int N, const int32_t* dims, int n_layers, const float* params, float p_drop, float* grads,
                                        void* workspace, size_t workspace_bytes, sq_stream_t stream) {
    HePlan P;
    if (int e = he_plan("he2rna_train_backward", dims, n_layers, B, N, &P)) return e;
    SQ_REQUIRE(params && grads && workspace, "he2rna_train_backward: null pointer");
    SQ_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "he2rna_train_backward: dropout p = %g must be in [0, 1) (p >= 1 drops every unit)", (double)p_drop);
    SQ_REQUIRE((((uintptr_t)workspace | (uintptr_t)params | (uintptr_t)grads) & 15) == 0,
               "he2rna_train_backward: params, grads and workspace must be 16-byte aligned");
    SQ_REQUIRE_WORKSPACE("he2rna_train_backward", workspace_bytes, P.bytes);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int M = P.M, L = P.L;
    const float* dy = ws + P.gscores;
    for (int i = L - 1; i >= 0; --i) {
        const int n_out = dims[i + 1], k_pad = P.ld[i], lddy = P.ld[i + 1];
        if (int e = sq_linear_weight_grad(SQ_F32, dy, lddy, ws + P.act[i], k_pad, grads + P.w_off[i], k_pad, grads + P.b_off[i], n_out,
                                          k_pad, M, ws + P.gemm, HE_GEMM_WS_BYTES, stream)) return e;
        if (i == 0) break;                           // the input needs no gradient
        float* wt = ws + P.wt;                       // W^T [k_pad, lddy], rows of the contraction zero-padded
        if (int e = sq_k_transpose(params + P.w_off[i], k_pad, wt, lddy, n_out, k_pad, 4, 1, 0, 0, st)) return e;
        float* dx = ws + P.dx[i & 1];
        if (int e = sq_linear(SQ_F32, dy, lddy, wt, lddy, nullptr, nullptr, 0, SQ_F32, SQ_ACT_NONE, dx, SQ_F32, k_pad, M, k_pad, lddy,
                              ws + P.gemm, HE_GEMM_WS_BYTES, stream)) return e;
        if (int e = launch_elementwise(true, dx, k_pad, ws + P.act[i], k_pad, M, dims[i], p_drop, 0, 0, 0, st)) return e;
        dy = dx;
    }
    return SQ_OK;
}
