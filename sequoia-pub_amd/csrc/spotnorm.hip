// Normalisation of raw spatial-transcriptomics spots on the device (include/sequoia_hip.h, "Spot normalisation"): the first
// lines of spatial_vis/get_emd.py (:148-155) -- sc.pp.normalize_total, sc.pp.log1p, sc.pp.scale and adata[:, gene].X --
// restated in f64 over a CSR matrix [n_spots, n_genes].
//   counts   c_i = sum_j X_ij.  One wave per row: lane l adds the entries l, l + 64, ... of the row in that order, the 64
//            partials meet in an xor butterfly (a + b is b + a, so every lane ends with the same sum).  The same pass checks
//            the row: strictly increasing indices inside [0, n_genes), non-negative finite values.
//   target   np.median(c[c > 0]).  The counts are sorted in chunks by cs_sort_chunks (colsort.hip); the k-th smallest is
//            the smallest bit pattern b with #(keys <= b) >= k + 1 -- non-negative doubles order as their bit patterns --
//            found by bisection, every count an upper-bound search (cs_first_gt) in each chunk.  No second sort.
//   log      L[i][c] = log1p(X[i][cols[c]] / s_i), s_i = (c_i + (c_i == 0)) / after.  A column list: one thread per
//            (row, column) searches the row's sorted indices; all genes: zero-fill, then every row scatters its entries.
//   scale    per column mean, two-pass standard deviation (ddof 1) and z = (l - mean) / sd in place.  16 consecutive
//            columns x 16 row lanes per workgroup; a lane adds every 16th row in row order, the 16 lanes meet in an LDS
//            tree.
// Separately rounded f64 operations in a fixed order; the only atomics are integer (the status word, counters in LDS).
#include "../../include/sequoia_hip.h"
#include "colsort.h"

#pragma clang fp contract(off)      // (l - m) (l - m) and every sum are separately rounded operations

namespace {

constexpr int SN_ROW_THREADS = 256;       // four waves, one row each
constexpr int SN_ROWS_PER_BLOCK = SN_ROW_THREADS / 64;
constexpr int SN_TARGET_THREADS = 256;
constexpr int SN_COL_THREADS = 256;
constexpr int SN_SCALE_COLS = 16;         // consecutive columns of one workgroup: 128 B of every row
constexpr int SN_SCALE_LANES = 16;        // row lanes per column

template <typename T>
__device__ __forceinline__ double sn_value(const void* data, long long p) { return (double)((const T*)data)[p]; }

__device__ __forceinline__ double sn_load(const void* data, int kind, long long p) {
    return kind == SQ_SN_DATA_F64 ? sn_value<double>(data, p) : kind == SQ_SN_DATA_F32 ? sn_value<float>(data, p) : sn_value<int32_t>(data, p);
}

// the row's [start, end) if it lies inside [0, nnz], else an empty range (and false)
__device__ __forceinline__ bool sn_row(const int64_t* __restrict__ indptr, int i, long long nnz, long long& s, long long& e) {
    s = indptr[i];
    e = indptr[i + 1];
    if (s >= 0 && s <= e && e <= nnz) return true;
    s = e = 0;
    return false;
}

// ------------------------------------------------------------------------------------------
// 1. counts per spot
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_ROW_THREADS) void sn_counts_kernel(const void* __restrict__ data, int kind, const int32_t* __restrict__ indices,
                                                                    const int64_t* __restrict__ indptr, int n_spots, int n_genes, long long nnz,
                                                                    double* __restrict__ counts, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * SN_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n_spots) return;                                 // the whole wave leaves
    long long s, e;
    int bad = sn_row(indptr, i, nnz, s, e) ? 0 : SQ_SN_BAD_INDPTR;
    double part = 0.0;
    for (long long p = s + lane; p < e; p += 64) {
        const int j = indices[p];
        const double v = sn_load(data, kind, p);
        if (j < 0 || j >= n_genes) bad |= SQ_SN_BAD_INDEX;
        if (p > s && indices[p - 1] >= j) bad |= SQ_SN_BAD_ORDER;
        if (!(v >= 0.0) || v == INFINITY) bad |= SQ_SN_BAD_VALUE;
        part += v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) counts[i] = part;
    if (bad) atomicOr(status, bad);                           // an integer atomic
}

// ------------------------------------------------------------------------------------------
// 2. the median of the positive counts
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ long long sn_block_sum(long long v, long long* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous sum has been read
    red[tid] = v;
    __syncthreads();
    for (int off = SN_TARGET_THREADS >> 1; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    return red[0];
}

// #(keys <= x) over the sorted chunks; thread t owns the chunks t, t + THREADS, ...
__device__ __forceinline__ long long sn_count_le(const double* __restrict__ sorted, const int32_t* __restrict__ valid, int chunks, double x,
                                                 long long* red) {
    long long mine = 0;
    for (int k = threadIdx.x; k < chunks; k += SN_TARGET_THREADS) mine += cs_first_gt(sorted + (size_t)k * CS_CHUNK, 0, valid[k], x);
    return sn_block_sum(mine, red);
}

// the key of 0-based rank r: the smallest non-negative bit pattern b with #(keys <= b) > r
__device__ __forceinline__ double sn_select(const double* __restrict__ sorted, const int32_t* __restrict__ valid, int chunks, long long r,
                                            long long* red) {
    unsigned long long lo = 0, hi = 0x7FF0000000000000ull;    // 0.0 .. +inf
    while (lo < hi) {                                         // uniform over the workgroup: every thread holds the same lo, hi
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (sn_count_le(sorted, valid, chunks, __longlong_as_double((long long)mid), red) > r) hi = mid;
        else lo = mid + 1;
    }
    return __longlong_as_double((long long)lo);
}

__global__ __launch_bounds__(SN_TARGET_THREADS) void sn_target_kernel(const double* __restrict__ sorted, const int32_t* __restrict__ valid, int chunks,
                                                                       double* __restrict__ after, int32_t* __restrict__ n_positive) {
    __shared__ long long red[SN_TARGET_THREADS];
    long long mine = 0;
    for (int k = threadIdx.x; k < chunks; k += SN_TARGET_THREADS) mine += valid[k];
    const long long total = sn_block_sum(mine, red);          // the keys that are numbers (a NaN count sorts behind them)
    const long long zeros = sn_count_le(sorted, valid, chunks, 0.0, red);
    const long long npos = total - zeros;
    double med = __builtin_nan("");
    if (npos > 0) {
        const double a = sn_select(sorted, valid, chunks, zeros + (npos - 1) / 2, red);
        med = a;
        if ((npos & 1) == 0) {
            const double b = sn_select(sorted, valid, chunks, zeros + npos / 2, red);
            med = (a + b) / 2.0;
        }
    }
    if (threadIdx.x == 0) {
        after[0] = med;
        n_positive[0] = (int32_t)npos;
    }
}

// ------------------------------------------------------------------------------------------
// 3. log1p of the normalised columns
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double sn_size_factor(double c, double after) { return (c + (c == 0.0 ? 1.0 : 0.0)) / after; }

// consecutive threads on consecutive columns of one row: the stores of a wave are one run
__global__ __launch_bounds__(SN_COL_THREADS) void sn_log_cols_kernel(const void* __restrict__ data, int kind, const int32_t* __restrict__ indices,
                                                                      const int64_t* __restrict__ indptr, int n_spots, long long nnz,
                                                                      const double* __restrict__ counts, const double* __restrict__ after,
                                                                      const int32_t* __restrict__ cols, int C, double* __restrict__ L) {
    const size_t total = (size_t)n_spots * (size_t)C;
    const double aft = after[0];
    for (size_t t = (size_t)blockIdx.x * SN_COL_THREADS + threadIdx.x; t < total; t += (size_t)gridDim.x * SN_COL_THREADS) {
        const size_t i = t / (size_t)C;
        const int g = cols[t - i * (size_t)C];
        long long lo, hi;
        sn_row(indptr, (int)i, nnz, lo, hi);
        const long long end = hi;
        while (lo < hi) {                                     // first index >= g
            const long long mid = (lo + hi) >> 1;
            if (indices[mid] < g) lo = mid + 1; else hi = mid;
        }
        double l = 0.0;
        if (lo < end && indices[lo] == g) l = log1p(sn_load(data, kind, lo) / sn_size_factor(counts[i], aft));
        L[t] = l;
    }
}

// all genes: L is zero; a wave per row stores the row's entries (an index outside [0, n_genes) is stored nowhere)
__global__ __launch_bounds__(SN_ROW_THREADS) void sn_log_scatter_kernel(const void* __restrict__ data, int kind, const int32_t* __restrict__ indices,
                                                                         const int64_t* __restrict__ indptr, int n_spots, int n_genes, long long nnz,
                                                                         const double* __restrict__ counts, const double* __restrict__ after,
                                                                         double* __restrict__ L) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * SN_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n_spots) return;
    long long s, e;
    sn_row(indptr, i, nnz, s, e);
    const double sf = sn_size_factor(counts[i], after[0]);
    double* const row = L + (size_t)i * (size_t)n_genes;
    for (long long p = s + lane; p < e; p += 64) {
        const int j = indices[p];
        if (j >= 0 && j < n_genes) row[j] = log1p(sn_load(data, kind, p) / sf);
    }
}

// ------------------------------------------------------------------------------------------
// 4. scale: mean, standard deviation, z
// ------------------------------------------------------------------------------------------
// the 16 lanes' partials of every column in fixed order: (((0 + 8) + (4 + 12)) + ...) as the halving tree gives them
__device__ __forceinline__ double sn_lane_tree(double v, double (*red)[SN_SCALE_COLS], int cx, int ry) {
    __syncthreads();                                          // the previous tree has been read
    red[ry][cx] = v;
    __syncthreads();
    for (int off = SN_SCALE_LANES >> 1; off > 0; off >>= 1) {
        if (ry < off) red[ry][cx] += red[ry + off][cx];
        __syncthreads();
    }
    return red[0][cx];
}

__global__ __launch_bounds__(SN_SCALE_COLS * SN_SCALE_LANES) void sn_scale_kernel(double* __restrict__ L, int n, int ld, int C, double* __restrict__ mean,
                                                                                   double* __restrict__ sd, int write_z) {
    __shared__ double red[SN_SCALE_LANES][SN_SCALE_COLS];
    const int cx = threadIdx.x % SN_SCALE_COLS, ry = threadIdx.x / SN_SCALE_COLS;
    const int c = blockIdx.x * SN_SCALE_COLS + cx;
    const bool in = c < C;                                    // threads beyond the last column add zeros and store nothing
    double* const col = L + (in ? c : 0);
    double part = 0.0;
    if (in)
        for (int i = ry; i < n; i += SN_SCALE_LANES) part += col[(size_t)i * (size_t)ld];
    const double m = sn_lane_tree(part, red, cx, ry) / (double)n;
    part = 0.0;
    if (in)
        for (int i = ry; i < n; i += SN_SCALE_LANES) {
            const double d = col[(size_t)i * (size_t)ld] - m;
            part += d * d;
        }
    double s = __dsqrt_rn(sn_lane_tree(part, red, cx, ry) / (double)(n - 1));
    if (s == 0.0) s = 1.0;
    if (!in) return;
    if (ry == 0) {
        mean[c] = m;
        sd[c] = s;
    }
    if (write_z)
        for (int i = ry; i < n; i += SN_SCALE_LANES) {
            double* const x = col + (size_t)i * (size_t)ld;
            *x = (*x - m) / s;
        }
}

bool sn_csr_ok(const char* name, const void* data, int data_kind, const int32_t* indices, const int64_t* indptr, int n_spots, int n_genes,
               long long nnz) {
    if (n_spots < 1 || n_spots > SQ_GT_MAX_SPOTS) {
        sq_set_error("%s: n_spots = %d, must be in 1..%d", name, n_spots, SQ_GT_MAX_SPOTS);
        return false;
    }
    if (n_genes < 1 || n_genes > SQ_SN_MAX_GENES) {
        sq_set_error("%s: n_genes = %d, must be in 1..%d", name, n_genes, SQ_SN_MAX_GENES);
        return false;
    }
    if (nnz < 0 || nnz > SQ_SN_MAX_NNZ) {
        sq_set_error("%s: nnz = %lld, must be in 0..%d", name, nnz, SQ_SN_MAX_NNZ);
        return false;
    }
    if (data_kind != SQ_SN_DATA_F32 && data_kind != SQ_SN_DATA_F64 && data_kind != SQ_SN_DATA_I32) {
        sq_set_error("%s: data_kind = %d, must be 0 (f32), 1 (f64) or 2 (int32)", name, data_kind);
        return false;
    }
    if (!indptr || (nnz > 0 && (!data || !indices))) {
        sq_set_error("%s: null data, indices or indptr pointer", name);
        return false;
    }
    if (((uintptr_t)data & (data_kind == SQ_SN_DATA_F64 ? 7 : 3)) || ((uintptr_t)indices & 3) || ((uintptr_t)indptr & 7)) {
        sq_set_error("%s: misaligned pointer", name);
        return false;
    }
    return true;
}

}  // namespace

static_assert(SN_SCALE_COLS * SN_SCALE_LANES <= 1024 && (SN_SCALE_LANES & (SN_SCALE_LANES - 1)) == 0, "the lane tree halves a power of two");
static_assert((SN_TARGET_THREADS & (SN_TARGET_THREADS - 1)) == 0, "the block sum halves a power of two");

extern "C" int sq_spot_counts(const void* data, int data_kind, const int32_t* indices, const int64_t* indptr, int n_spots, int n_genes,
                              long long nnz, double* counts, int32_t* status, sq_stream_t stream_) {
    if (!sn_csr_ok("spot_counts", data, data_kind, indices, indptr, n_spots, n_genes, nnz)) return SQ_ERR_ARG;
    SQ_REQUIRE(counts && status, "spot_counts: null counts or status pointer");
    SQ_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)status & 3) == 0, "spot_counts: misaligned pointer");
    hipStream_t st = (hipStream_t)stream_;
    SQ_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(sn_counts_kernel, dim3((unsigned)((n_spots + SN_ROWS_PER_BLOCK - 1) / SN_ROWS_PER_BLOCK)), dim3(SN_ROW_THREADS), 0, st, data,
                       data_kind, indices, indptr, n_spots, n_genes, nnz, counts, status);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_spot_target_workspace_bytes(int n_spots) {
    if (n_spots < 1 || n_spots > SQ_GT_MAX_SPOTS) return 0;
    const int chunks = cs_chunks(n_spots);
    return sq_align_up((size_t)chunks * CS_CHUNK * 8, 256) + sq_align_up((size_t)chunks * 4, 256) + 256;
}

extern "C" int sq_spot_target(const double* counts, int n_spots, double* after, int32_t* n_positive, void* workspace, size_t workspace_bytes,
                              sq_stream_t stream_) {
    SQ_REQUIRE(n_spots >= 1 && n_spots <= SQ_GT_MAX_SPOTS, "spot_target: n_spots = %d, must be in 1..%d", n_spots, SQ_GT_MAX_SPOTS);
    SQ_REQUIRE(counts && after && n_positive && workspace, "spot_target: null counts, after, n_positive or workspace pointer");
    SQ_REQUIRE((((uintptr_t)counts | (uintptr_t)after | (uintptr_t)workspace) & 7) == 0 && ((uintptr_t)n_positive & 3) == 0,
               "spot_target: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("spot_target", workspace_bytes, sq_spot_target_workspace_bytes(n_spots));
    hipStream_t st = (hipStream_t)stream_;
    const int chunks = cs_chunks(n_spots);
    char* const ws = (char*)workspace;
    double* const sorted = (double*)ws;
    int32_t* const valid = (int32_t*)(ws + sq_align_up((size_t)chunks * CS_CHUNK * 8, 256));
    int32_t* const nan_flag = (int32_t*)((char*)valid + sq_align_up((size_t)chunks * 4, 256));
    if (int e = cs_sort_chunks(counts, 1, n_spots, 1, nullptr, 1, sorted, valid, nan_flag, st)) return e;
    hipLaunchKernelGGL(sn_target_kernel, dim3(1), dim3(SN_TARGET_THREADS), 0, st, (const double*)sorted, (const int32_t*)valid, chunks, after,
                       n_positive);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_spot_log_columns(const void* data, int data_kind, const int32_t* indices, const int64_t* indptr, int n_spots, int n_genes,
                                   long long nnz, const double* counts, const double* after, const int32_t* cols, int C, double* L,
                                   sq_stream_t stream_) {
    if (!sn_csr_ok("spot_log_columns", data, data_kind, indices, indptr, n_spots, n_genes, nnz)) return SQ_ERR_ARG;
    SQ_REQUIRE(C >= 1 && (cols || C == n_genes), "spot_log_columns: C = %d columns, must be at least 1 and, without a column list, n_genes = %d", C,
               n_genes);
    SQ_REQUIRE((long long)n_spots * (long long)C <= SQ_SN_MAX_CELLS, "spot_log_columns: n_spots C = %lld cells, must be at most %d",
               (long long)n_spots * (long long)C, SQ_SN_MAX_CELLS);
    SQ_REQUIRE(counts && after && L, "spot_log_columns: null counts, after or L pointer");
    SQ_REQUIRE((((uintptr_t)counts | (uintptr_t)after | (uintptr_t)L) & 7) == 0 && ((uintptr_t)cols & 3) == 0, "spot_log_columns: misaligned pointer");
    hipStream_t st = (hipStream_t)stream_;
    if (cols) {
        hipLaunchKernelGGL(sn_log_cols_kernel, dim3(cs_blocks((size_t)n_spots * (size_t)C, SN_COL_THREADS)), dim3(SN_COL_THREADS), 0, st, data, data_kind,
                           indices, indptr, n_spots, nnz, counts, after, cols, C, L);
    } else {
        SQ_HIP_CHECK(hipMemsetAsync(L, 0, (size_t)n_spots * (size_t)n_genes * 8, st));
        hipLaunchKernelGGL(sn_log_scatter_kernel, dim3((unsigned)((n_spots + SN_ROWS_PER_BLOCK - 1) / SN_ROWS_PER_BLOCK)), dim3(SN_ROW_THREADS), 0, st,
                           data, data_kind, indices, indptr, n_spots, n_genes, nnz, counts, after, L);
    }
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_spot_scale(double* L, int n, int ld, int C, double* mean, double* sd, int write_z, sq_stream_t stream_) {
    SQ_REQUIRE_TABLE("spot_scale", n, 2, SQ_GT_MAX_SPOTS, "C", C, 0, ld, nullptr);
    SQ_REQUIRE(write_z == 0 || write_z == 1, "spot_scale: write_z = %d, must be 0 or 1", write_z);
    SQ_REQUIRE(L && mean && sd, "spot_scale: null L, mean or sd pointer");
    SQ_REQUIRE((((uintptr_t)L | (uintptr_t)mean | (uintptr_t)sd) & 7) == 0, "spot_scale: misaligned pointer");
    hipLaunchKernelGGL(sn_scale_kernel, dim3((unsigned)((C + SN_SCALE_COLS - 1) / SN_SCALE_COLS)), dim3(SN_SCALE_COLS * SN_SCALE_LANES), 0,
                       (hipStream_t)stream_, L, n, ld, C, mean, sd, write_z);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
