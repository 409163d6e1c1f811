// Map statistics of a predicted slide on the device (include/sequoia_hip.h, "Map statistics"): the numeric part of
// spatial_vis/gbm_celltype_analysis.py and the percentile step of spatial_vis/get_emd.py.
//   percentile   score2percentile (gbm_celltype_analysis.py:12-16,107; get_emd.py:21-25,172,175): the reference calls
//                scipy.stats.percentileofscore(column, x) once per row, O(n) each.  Here a column is cut into chunks of
//                CS_CHUNK rows that cs_sort_chunks (colsort.h, colsort.hip: the LDS bitonic sort, keys only) sorts into the
//                workspace; every element then takes a lower- and an upper-bound binary search (colsort.h) in every sorted
//                chunk of its column (a workgroup stages the chunk in LDS for 1024 elements).  #(column < x) and
//                #(column <= x) add over chunks, so nothing is merged.  Keys keep the input's type (f32 or f64) and are
//                compared as IEEE numbers, so -0.0 ties with 0.0 as it does in numpy.  A NaN is stored as +inf, as the pad
//                keys of a short chunk are, and raises the column's flag: a search only looks at the chunk's first `len`
//                keys (pads sort behind or beside every real key), and a flagged column comes back all NaN (scipy's
//                nan_policy='propagate').
//   means        df[genes of category].mean(axis=1) (:105): one thread per (tile, category), f64 sum in list order.
//   correlation  df[all_genes].corr() (:75): f64 column means (row slices added in slice order), then C = Z^T Z of the
//                centred columns on v_mfma_f64_16x16x4_f64 -- the TN form of km_dgemm_nt_kernel (kmeans.hip): a chunk of 32
//                table rows x 64 columns loads coalesced and lands in LDS as [k][column], centred on load.  Blocks on and
//                above the diagonal only; the rows are cut into slices (grid z) when there are few blocks, each slice
//                writes its partial C plane and the last kernel adds the planes in slice order, divides by
//                sqrt(C_ii) sqrt(C_jj), clips, and stores [i][j] and [j][i] from the same value.
// No floating-point atomics (the chunk sort counts a chunk's NaNs with an integer add in LDS) and no order that depends on
// scheduling: two calls give the same bytes.
#include "../../include/sequoia_hip.h"
#include "colsort.h"

#pragma clang fp contract(off)      // the sums and quotients the tests hold to numpy are separately rounded operations

namespace {

// ------------------------------------------------------------------------------------------
// 1. percentile of score
// ------------------------------------------------------------------------------------------
constexpr int MR_QROWS = 1024;            // query rows of one workgroup of the rank kernel

// grid (C, row blocks): a workgroup takes MR_QROWS rows of one column as queries (MR_QROWS / 256 per thread, in registers) and
// walks the column's sorted chunks through LDS, so every step of a search is an LDS read and a chunk is read from memory once
// per MR_QROWS queries (coalesced).  Neighbouring blocks hold neighbouring columns of the same rows, as in the chunk sort.
template <typename T>
__global__ __launch_bounds__(256) void map_rank_kernel(const T* __restrict__ values, int n, int ld, const int32_t* __restrict__ cols,
                                                       int C, const T* __restrict__ sorted, int npad,
                                                       const int32_t* __restrict__ nan_flag, double scale, double* __restrict__ out) {
    __shared__ T key[CS_CHUNK];
    constexpr int Q = MR_QROWS / 256;
    const int c = blockIdx.x, row0 = blockIdx.y * MR_QROWS, tid = threadIdx.x;
    const bool flagged = nan_flag[c] != 0;                  // the same for the whole workgroup
    const int col = cols ? cols[c] : c;
    T x[Q];
    int left[Q], right[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = row0 + q * 256 + tid;
        x[q] = i < n && !flagged ? values[(size_t)i * (size_t)ld + (size_t)col] : (T)0;
        left[q] = right[q] = 0;
    }
    const T* const s = sorted + (size_t)c * (size_t)npad;
    for (int r0 = 0; r0 < n && !flagged; r0 += CS_CHUNK) {
        const int len = min(CS_CHUNK, n - r0);
        __syncthreads();                                    // the previous chunk's searches are done
        for (int i = tid; i < len; i += 256) key[i] = s[r0 + i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int lo = cs_first_ge(key, len, x[q]);
            left[q] += lo;
            right[q] += cs_first_gt(key, lo, len, x[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = row0 + q * 256 + tid;
        if (i < n)
            out[(size_t)i * (size_t)C + c] = flagged ? __builtin_nan("") : (double)(left[q] + right[q] + (left[q] < right[q] ? 1 : 0)) * scale;
    }
}

// idxmax(axis=1): the first column holding the row's largest value, NaN skipped, -1 for a row of NaN
__global__ __launch_bounds__(256) void map_row_argmax_kernel(const double* __restrict__ perc, int n, int C, int32_t* __restrict__ argmax) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* const row = perc + (size_t)i * (size_t)C;
    int best = -1;
    double bv = 0.0;
    for (int c = 0; c < C; ++c) {
        const double v = row[c];
        if (v == v && (best < 0 || v > bv)) { best = c; bv = v; }
    }
    argmax[i] = best;
}

// workspace: the sorted chunks of the C columns, then the columns' NaN flags
size_t mr_sorted_bytes(int n, int C, int values_f64) { return sq_align_up((size_t)C * (size_t)cs_chunks(n) * CS_CHUNK * (values_f64 ? 8 : 4), 256); }

template <typename T>
int mr_rank(const void* values, int n, int ld, const int32_t* cols, int C, double scale, double* out, const void* sorted,
            const int32_t* nan_flag, hipStream_t st) {
    hipLaunchKernelGGL(map_rank_kernel<T>, dim3((unsigned)C, (unsigned)((n + MR_QROWS - 1) / MR_QROWS)), dim3(256), 0, st, (const T*)values, n, ld,
                       cols, C, (const T*)sorted, cs_chunks(n) * CS_CHUNK, nan_flag, scale, out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

// ------------------------------------------------------------------------------------------
// 2. category means
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_category_means_kernel(const float* __restrict__ pred, int n, int ld,
                                                                 const int32_t* __restrict__ members, const int32_t* __restrict__ offsets,
                                                                 int n_cat, double* __restrict__ out) {
    const size_t total = (size_t)n * (size_t)n_cat;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t i = idx / (size_t)n_cat;
        const int cat = (int)(idx - i * (size_t)n_cat);
        const int b = offsets[cat], e = offsets[cat + 1];
        const float* const row = pred + i * (size_t)ld;
        double s = 0.0;
        for (int j = b; j < e; ++j) s += (double)row[members[j]];
        out[idx] = e > b ? s / (double)(e - b) : __builtin_nan("");
    }
}

// ------------------------------------------------------------------------------------------
// 3. gene-gene Pearson correlation
// ------------------------------------------------------------------------------------------
constexpr int MC_TILE = 64;               // output block: 64 x 64, 4 waves x (2 x 2 tiles of 16 x 16)
constexpr int MC_KC = 32;                 // table rows per LDS chunk
constexpr int MC_SUM_ROWS = 256;          // rows per slice of the column sums (at most MC_SUM_SLICES slices)
constexpr int MC_SUM_SLICES = 256;
constexpr int MC_TARGET_BLOCKS = 512;     // row slices of the Gram product until about this many blocks run

struct McPlan {
    int T;              // 64-column blocks per side
    int S, rper;        // Gram row slices, rows per slice (a multiple of MC_KC)
    int R, sum_rows;    // column-sum row slices, rows per slice
    size_t off_mean, off_ss, off_flag, off_psum, off_part, bytes;
};

McPlan mc_plan(int n, int K) {
    McPlan p;
    p.T = (K + MC_TILE - 1) / MC_TILE;
    const long long blocks = (long long)p.T * (p.T + 1) / 2;
    long long want = (MC_TARGET_BLOCKS + blocks - 1) / blocks;
    const int most = (n + 4 * MC_KC - 1) / (4 * MC_KC);                    // a slice has at least 128 rows
    const int S0 = (int)(want < 1 ? 1 : (want > most ? most : want));
    p.rper = ((n + S0 - 1) / S0 + MC_KC - 1) / MC_KC * MC_KC;
    p.S = (n + p.rper - 1) / p.rper;
    p.R = (n + MC_SUM_ROWS - 1) / MC_SUM_ROWS;
    if (p.R > MC_SUM_SLICES) p.R = MC_SUM_SLICES;
    p.sum_rows = (n + p.R - 1) / p.R;
    p.R = (n + p.sum_rows - 1) / p.sum_rows;
    size_t o = 0;
    p.off_mean = o; o += sq_align_up((size_t)K * 8, 256);
    p.off_ss = o;   o += sq_align_up((size_t)K * 8, 256);
    p.off_flag = o; o += sq_align_up((size_t)K * 4, 256);
    p.off_psum = o; o += sq_align_up((size_t)p.R * (size_t)K * 8, 256);
    p.off_part = o; o += p.S > 1 ? sq_align_up((size_t)p.S * (size_t)K * (size_t)K * 8, 256) : 0;     // one slice: straight into `out`
    p.bytes = o;
    return p;
}

// grid (ceil(K / 256), R): a lane per column (coalesced across columns), a slice of rows per block
__global__ __launch_bounds__(256) void map_col_sum_kernel(const float* __restrict__ pred, int n, int ld, const int32_t* __restrict__ cols,
                                                          int K, int sum_rows, double* __restrict__ psum, int32_t* __restrict__ varies) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    const int col = cols ? cols[j] : j;
    const int r_lo = blockIdx.y * sum_rows, r_hi = min(n, r_lo + sum_rows);
    const float x0 = pred[col];
    double s = 0.0;
    bool v = false;
    for (int r = r_lo; r < r_hi; ++r) {
        const float x = pred[(size_t)r * (size_t)ld + (size_t)col];
        s += (double)x;
        v = v || x != x0;
    }
    psum[(size_t)blockIdx.y * (size_t)K + j] = s;
    if (v) varies[j] = 1;                  // every writer stores the same value
}

__global__ __launch_bounds__(256) void map_col_mean_kernel(const double* __restrict__ psum, int K, int R, int n, double* __restrict__ mean) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += psum[(size_t)r * (size_t)K + j];
    mean[j] = s / (double)n;
}

// part[slice][i][j] = sum over the slice's rows of z_i z_j, z = (double)x - mean, for the blocks with bx >= by
__global__ __launch_bounds__(256) void map_gram_tn_kernel(const float* __restrict__ pred, int n, int ld, const int32_t* __restrict__ cols,
                                                          int K, const double* __restrict__ mean, int rper, double* __restrict__ part) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double sa[MC_KC][MC_TILE + 2];
    __shared__ double sb[MC_KC][MC_TILE + 2];
    const bool diag = blockIdx.x == blockIdx.y;
    const int m0 = blockIdx.y * MC_TILE, n0 = blockIdx.x * MC_TILE;
    const int r_lo = blockIdx.z * rper, r_hi = min(n, r_lo + rper);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // loader: a thread owns one column of each operand block and rows lr, lr + 4, ... of a chunk: a wave reads 64
    // neighbouring columns of one table row
    const int lc = tid & 63, lr = tid >> 6;
    const bool a_in = m0 + lc < K, b_in = !diag && n0 + lc < K;
    const size_t a_col = a_in ? (size_t)(cols ? cols[m0 + lc] : m0 + lc) : 0, b_col = b_in ? (size_t)(cols ? cols[n0 + lc] : n0 + lc) : 0;
    const double a_mean = a_in ? mean[m0 + lc] : 0.0, b_mean = b_in ? mean[n0 + lc] : 0.0;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    float va[MC_KC / 4], vb[MC_KC / 4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < MC_KC / 4; ++p) {
            const int r = k0 + lr + 4 * p;
            const bool row_in = r < r_hi;
            const size_t base = (size_t)(row_in ? r : 0) * (size_t)ld;
            va[p] = a_in && row_in ? pred[base + a_col] : 0.0f;
            vb[p] = b_in && row_in ? pred[base + b_col] : 0.0f;
        }
    };
    const double (*const pb)[MC_TILE + 2] = diag ? sa : sb;
    if (r_lo < r_hi) fetch(r_lo);
    for (int k0 = r_lo; k0 < r_hi; k0 += MC_KC) {
#pragma unroll
        for (int p = 0; p < MC_KC / 4; ++p) {
            const bool row_in = k0 + lr + 4 * p < r_hi;        // rows beyond the slice and columns beyond K are zeros, not -mean
            sa[lr + 4 * p][lc] = a_in && row_in ? (double)va[p] - a_mean : 0.0;
            if (!diag) sb[lr + 4 * p][lc] = b_in && row_in ? (double)vb[p] - b_mean : 0.0;
        }
        __syncthreads();
        if (k0 + MC_KC < r_hi) fetch(k0 + MC_KC);
#pragma unroll
        for (int ks = 0; ks < MC_KC; ks += 4) {
            const int k = ks + (lane >> 4);
            double fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = sa[k][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = pb[k][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* const plane = part + (size_t)blockIdx.z * (size_t)K * (size_t)K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + i * 16 + (lane >> 4) + 4 * r;
                const int nn = n0 + wn * 32 + j * 16 + (lane & 15);
                if (m < K && nn < K) plane[(size_t)m * (size_t)K + nn] = acc[i][j][r];
            }
}

__global__ __launch_bounds__(256) void map_corr_diag_kernel(const double* __restrict__ part, int K, int S, double* __restrict__ ss) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    double s = 0.0;
    for (int z = 0; z < S; ++z) s += part[((size_t)z * (size_t)K + j) * (size_t)K + j];
    ss[j] = s;
}

// grid (T, T), blocks with bx >= by: the slices of C_ij added in order, the quotient, both stores from one value.  `part`
// may be `out` (one slice): a block reads its own block's upper entries before the barrier and writes after it, and no
// other block reads what it writes.
__global__ __launch_bounds__(256) void map_corr_finish_kernel(const double* part, int K, int S, const double* __restrict__ ss,
                                                              const int32_t* __restrict__ varies, double* out) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double tile[MC_TILE][MC_TILE + 1];
    const bool diag = blockIdx.x == blockIdx.y;
    const int i0 = blockIdx.y * MC_TILE, j0 = blockIdx.x * MC_TILE;
    const int jj = threadIdx.x & 63;
    for (int ii = threadIdx.x >> 6; ii < MC_TILE; ii += 4) {
        const int i = i0 + ii, j = j0 + jj;
        if (i >= K || j >= K || (diag && jj < ii)) continue;
        double c = 0.0;
        for (int z = 0; z < S; ++z) c += part[((size_t)z * (size_t)K + i) * (size_t)K + j];
        const double si = ss[i], sj = ss[j];
        double r = c / (sqrt(si) * sqrt(sj));
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
        if (i == j && si == si) r = 1.0;
        if (!varies[i] || !varies[j]) r = __builtin_nan("");
        tile[ii][jj] = r;
    }
    __syncthreads();
    for (int ii = threadIdx.x >> 6; ii < MC_TILE; ii += 4) {
        if (diag) {
            if (i0 + ii < K && j0 + jj < K) out[(size_t)(i0 + ii) * (size_t)K + j0 + jj] = jj >= ii ? tile[ii][jj] : tile[jj][ii];
        } else {
            if (i0 + ii < K && j0 + jj < K) out[(size_t)(i0 + ii) * (size_t)K + j0 + jj] = tile[ii][jj];
            if (j0 + ii < K && i0 + jj < K) out[(size_t)(j0 + ii) * (size_t)K + i0 + jj] = tile[jj][ii];
        }
    }
}

}  // namespace

static_assert(MC_KC % 4 == 0 && 256 / 64 * (MC_KC / 4) == MC_KC, "the loader's 4 rows x 64 columns per pass cover a chunk");

extern "C" int sq_map_rank_chunk_rows(void) { return CS_CHUNK; }

extern "C" size_t sq_map_percentile_workspace_bytes(int n, int C, int values_f64) {
    if (n < 1 || n > SQ_MAP_MAX_ROWS || C < 1 || (values_f64 != 0 && values_f64 != 1)) return 0;
    return mr_sorted_bytes(n, C, values_f64) + sq_align_up((size_t)C * 4, 256);
}

extern "C" int sq_map_percentile(const void* values, int values_f64, int n, int ld, const int32_t* cols, int C, double scale,
                                 double* out, int32_t* argmax, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE_TABLE("map_percentile", n, 1, SQ_MAP_MAX_ROWS, "C", C, 0, ld, cols);
    SQ_REQUIRE(values_f64 == 0 || values_f64 == 1, "map_percentile: values_f64 = %d, must be 0 (f32) or 1 (f64)", values_f64);
    SQ_REQUIRE(scale == scale, "map_percentile: scale is not a number");
    SQ_REQUIRE(values && out && workspace, "map_percentile: null values, out or workspace pointer");
    SQ_REQUIRE(((uintptr_t)values & (values_f64 ? 7 : 3)) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)cols & 3) == 0 &&
               ((uintptr_t)argmax & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "map_percentile: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("map_percentile", workspace_bytes, sq_map_percentile_workspace_bytes(n, C, values_f64));
    hipStream_t st = (hipStream_t)stream_;
    int32_t* const nan_flag = (int32_t*)((char*)workspace + mr_sorted_bytes(n, C, values_f64));
    if (int e = cs_sort_chunks(values, values_f64, n, ld, cols, C, workspace, nullptr, nan_flag, st)) return e;
    if (int e = values_f64 ? mr_rank<double>(values, n, ld, cols, C, scale, out, workspace, nan_flag, st)
                           : mr_rank<float>(values, n, ld, cols, C, scale, out, workspace, nan_flag, st)) return e;
    if (argmax) {
        hipLaunchKernelGGL(map_row_argmax_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)out, n, C, argmax);
        SQ_LAUNCH_CHECK();
    }
    return SQ_OK;
}

extern "C" int sq_map_category_means(const float* pred, int n, int ld, const int32_t* members, int n_members, const int32_t* offsets,
                                     int n_cat, double* out, sq_stream_t stream_) {
    SQ_REQUIRE_ROWS("map_category_means", n, 1, SQ_MAP_MAX_ROWS);
    SQ_REQUIRE(n_cat >= 1 && n_members >= 0 && ld >= 1, "map_category_means: n_cat = %d (at least 1), n_members = %d (at least 0), ld = %d (at least 1)",
               n_cat, n_members, ld);
    SQ_REQUIRE(pred && offsets && out && (members || n_members == 0), "map_category_means: null pred, members, offsets or out pointer");
    SQ_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)members & 3) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)out & 7) == 0,
               "map_category_means: misaligned pointer");
    hipLaunchKernelGGL(map_category_means_kernel, dim3(cs_blocks((size_t)n * (size_t)n_cat, 256)), dim3(256), 0, (hipStream_t)stream_, pred, n, ld,
                       members, offsets, n_cat, out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_map_gene_corr_workspace_bytes(int n, int K) {
    if (n < 2 || n > SQ_MAP_MAX_ROWS || K < 1 || K > SQ_MAP_MAX_CORR_COLS) return 0;
    return mc_plan(n, K).bytes;
}

extern "C" int sq_map_gene_corr(const float* pred, int n, int ld, const int32_t* cols, int K, double* out, void* workspace,
                                size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE_TABLE("map_gene_corr", n, 2, SQ_MAP_MAX_ROWS, "K", K, SQ_MAP_MAX_CORR_COLS, ld, cols);
    SQ_REQUIRE(pred && out && workspace, "map_gene_corr: null pred, out or workspace pointer");
    SQ_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)cols & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
               "map_gene_corr: misaligned pointer");
    const McPlan p = mc_plan(n, K);
    SQ_REQUIRE_WORKSPACE("map_gene_corr", workspace_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream_;
    char* const ws = (char*)workspace;
    double* const mean = (double*)(ws + p.off_mean);
    double* const ss = (double*)(ws + p.off_ss);
    int32_t* const varies = (int32_t*)(ws + p.off_flag);
    double* const psum = (double*)(ws + p.off_psum);
    double* const part = p.S > 1 ? (double*)(ws + p.off_part) : out;
    const unsigned kb = (unsigned)((K + 255) / 256);
    SQ_HIP_CHECK(hipMemsetAsync(varies, 0, (size_t)K * sizeof(int32_t), st));
    hipLaunchKernelGGL(map_col_sum_kernel, dim3(kb, (unsigned)p.R), dim3(256), 0, st, pred, n, ld, cols, K, p.sum_rows, psum, varies);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(map_col_mean_kernel, dim3(kb), dim3(256), 0, st, (const double*)psum, K, p.R, n, mean);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(map_gram_tn_kernel, dim3((unsigned)p.T, (unsigned)p.T, (unsigned)p.S), dim3(256), 0, st, pred, n, ld, cols, K,
                       (const double*)mean, p.rper, part);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(map_corr_diag_kernel, dim3(kb), dim3(256), 0, st, (const double*)part, K, p.S, ss);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(map_corr_finish_kernel, dim3((unsigned)p.T, (unsigned)p.T), dim3(256), 0, st, (const double*)part, K, p.S,
                       (const double*)ss, (const int32_t*)varies, out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
