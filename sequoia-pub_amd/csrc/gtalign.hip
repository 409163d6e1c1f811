// Alignment of a predicted slide with its spatial-transcriptomics ground truth on the device (include/sequoia_hip.h,
// "Ground-truth alignment"): get_average and median_filter of spatial_vis/get_emd.py and the np.unique counts of :204-205.
//   nearest spots  get_average (:27-32) sorts the distances of ALL spots for every tile and every gene; the k nearest do not
//                  depend on the gene, so they are found once.  One thread per tile; the spots pass through LDS in chunks of
//                  GT_SPOT_CHUNK (x, y) pairs that every lane reads at the same address (a broadcast); the k best are held in
//                  registers (k is a template parameter, every index static).  Spots are visited in index order, so a
//                  candidate has the highest index so far and enters only if its d is STRICTLY below the held k-th d, behind
//                  every held entry with d <= its own: the first k of Python's stable sort.  d = sqrt(dx dx + dy dy) with
//                  every operation rounded on its own; sqrt(a) < sqrt(b) implies a < b, so d^2 against the held k-th d^2 is
//                  a pre-filter and the square root is taken for the few candidates that pass it.
//   means          np.mean of the k kept values (:34-38): 0.0 + e0 + e1 + ... in kept order for k <= 7 and numpy's unrolled
//                  pairwise block ((e0+e1)+(e2+e3)) + ((e4+e5)+(e6+e7)) for k = 8, then / k.  One thread per (tile, column).
//   median filter  median_filter (:41-51): a first kernel scatters the row numbers into an int32 grid (-1 = empty cell), a
//                  second reads the (2r+1)^2 neighbour cells of every row and insertion-sorts the members' values in a
//                  per-thread column of LDS (element s of thread t at [s][t]: no bank conflict, no scratch).
//   unique         len(np.unique(column)) (:204-205): chunks of CS_CHUNK rows sorted by cs_sort_chunks (colsort.h, colsort.hip:
//                  the LDS bitonic sort the percentile shares), then a value counts where it first appears in its chunk and no
//                  EARLIER chunk holds it (earlier chunks walk through LDS, a binary search of colsort.h each).
// Integer work and separately rounded f64 operations in a fixed order; the only atomics are integer counters in LDS.  Two
// calls give the same bytes.
#include "../../include/sequoia_hip.h"
#include "colsort.h"

#pragma clang fp contract(off)      // dx dx + dy dy and every sum are separately rounded operations, as numpy's are

namespace {

constexpr int GT_SPOT_CHUNK = 2048;       // spots of one LDS chunk: 2048 x (x, y) f64 = 32 KiB
constexpr int GT_NS_THREADS = 64;         // one wave: a slide of a few thousand tiles still spreads over many CUs
constexpr int GT_MF_THREADS = 128;        // r = 3: 49 x 128 x 8 B = 49 KiB of LDS
constexpr int GT_UQ_COUNT_THREADS = 256;

// ------------------------------------------------------------------------------------------
// 1. nearest spots
// ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(GT_NS_THREADS) void gt_nearest_kernel(const double* __restrict__ xc, const double* __restrict__ yc, int n_tiles,
                                                                   const double* __restrict__ sx, const double* __restrict__ sy, int n_spots,
                                                                   int k_eff, int32_t* __restrict__ idx, double* __restrict__ dist) {
    __shared__ double2 sp[GT_SPOT_CHUNK];
    const int tid = threadIdx.x, t = blockIdx.x * GT_NS_THREADS + tid;
    const int tt = t < n_tiles ? t : n_tiles - 1;             // lanes beyond the last tile stage spots and store nothing
    const double x = xc[tt], y = yc[tt];
    double hd[K], h2[K];
    int hi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { hd[s] = INFINITY; h2[s] = INFINITY; hi[s] = -1; }
    for (int c0 = 0; c0 < n_spots; c0 += GT_SPOT_CHUNK) {
        const int len = min(GT_SPOT_CHUNK, n_spots - c0);
        __syncthreads();                                      // the previous chunk has been read
        for (int i = tid; i < len; i += GT_NS_THREADS) sp[i] = make_double2(sx[c0 + i], sy[c0 + i]);
        __syncthreads();
        for (int j = 0; j < len; ++j) {
            const double2 s = sp[j];
            const double dx = s.x - x, dy = s.y - y;
            const double d2 = dx * dx + dy * dy;
            const int g = c0 + j;
            if (g < K || d2 < h2[K - 1]) {                    // the first K spots always enter: the list is not full yet
                const double d = __dsqrt_rn(d2);
                if (g < K || d < hd[K - 1]) {
                    const int filled = g < K ? g : K;
                    int p = 0;                                // held entries with d <= the candidate's stay in front of it
#pragma unroll
                    for (int q = 0; q < K; ++q) p += (q < filled && hd[q] <= d) ? 1 : 0;
#pragma unroll
                    for (int q = K - 1; q >= 1; --q)
                        if (q > p) { hd[q] = hd[q - 1]; h2[q] = h2[q - 1]; hi[q] = hi[q - 1]; }
#pragma unroll
                    for (int q = 0; q < K; ++q)
                        if (q == p) { hd[q] = d; h2[q] = d2; hi[q] = g; }
                }
            }
        }
    }
    if (t >= n_tiles) return;
#pragma unroll
    for (int s = 0; s < K; ++s)
        if (s < k_eff) {
            idx[(size_t)t * (size_t)k_eff + s] = hi[s];
            if (dist) dist[(size_t)t * (size_t)k_eff + s] = hd[s];
        }
}

template <int K>
void gt_launch_nearest(const double* xc, const double* yc, int n_tiles, const double* sx, const double* sy, int n_spots, int k_eff,
                       int32_t* idx, double* dist, hipStream_t st) {
    hipLaunchKernelGGL(gt_nearest_kernel<K>, dim3((unsigned)((n_tiles + GT_NS_THREADS - 1) / GT_NS_THREADS)), dim3(GT_NS_THREADS), 0, st, xc, yc,
                       n_tiles, sx, sy, n_spots, k_eff, idx, dist);
}

// ------------------------------------------------------------------------------------------
// 2. means of the kept spots
// ------------------------------------------------------------------------------------------
// consecutive columns in consecutive lanes: the k gathers of a wave read k runs of neighbouring columns.  A spot index
// outside [0, n_spots) is not followed: the mean is NaN.
template <typename T>
__global__ __launch_bounds__(256) void gt_spot_means_kernel(const int32_t* __restrict__ idx, int n_tiles, int k_eff, const T* __restrict__ expr,
                                                            int n_spots, int ld, const int32_t* __restrict__ cols, int C,
                                                            double* __restrict__ out) {
    const size_t total = (size_t)n_tiles * (size_t)C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t i = e / (size_t)C;
        const int c = (int)(e - i * (size_t)C);
        const size_t col = (size_t)(cols ? cols[c] : c);
        const int32_t* const id = idx + i * (size_t)k_eff;
        double v[SQ_GT_MAX_K];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < SQ_GT_MAX_K; ++j) {
            v[j] = 0.0;
            if (j < k_eff) {
                const int g = id[j];
                const bool in = g >= 0 && g < n_spots;
                ok = ok && in;
                if (in) v[j] = (double)expr[(size_t)g * (size_t)ld + col];
            }
        }
        double s = 0.0;
        if (k_eff == 8) {
            s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));       // numpy's pairwise block of 8
        } else {
#pragma unroll
            for (int j = 0; j < SQ_GT_MAX_K - 1; ++j)
                if (j < k_eff) s += v[j];
        }
        out[e] = ok ? s / (double)k_eff : __builtin_nan("");
    }
}

// ------------------------------------------------------------------------------------------
// 3. median filter over the sparse tile grid
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gt_grid_scatter_kernel(const int32_t* __restrict__ xtf, const int32_t* __restrict__ ytf, int n, int gw,
                                                              int gh, int32_t* __restrict__ grid, uint8_t* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = xtf[i], y = ytf[i];
    if (x < 0 || x >= gw || y < 0 || y >= gh) { flag[0] = 1; return; }       // every writer stores the same value
    grid[(size_t)y * (size_t)gw + (size_t)x] = i;                           // two rows of one cell: one wins, the other finds out below
}

template <int R>
__global__ __launch_bounds__(GT_MF_THREADS) void gt_median_kernel(const double* __restrict__ values, int n, int ld, const int32_t* __restrict__ cols,
                                                                  int C, const int32_t* __restrict__ xtf, const int32_t* __restrict__ ytf, int gw,
                                                                  int gh, const int32_t* __restrict__ grid, int nan_absent,
                                                                  double* __restrict__ out, int32_t* __restrict__ counts,
                                                                  uint8_t* __restrict__ flag) {
    constexpr int M = (2 * R + 1) * (2 * R + 1), T = GT_MF_THREADS;
    __shared__ double buf[M * T];
    double* const mine = buf + threadIdx.x;                   // this thread's sorted values: element s at mine[s * T]
    const size_t total = (size_t)n * (size_t)C;
    for (size_t e = (size_t)blockIdx.x * T + threadIdx.x; e < total; e += (size_t)gridDim.x * T) {
        const size_t i = e / (size_t)C;
        const int c = (int)(e - i * (size_t)C);
        const size_t col = (size_t)(cols ? cols[c] : c);
        const int x = xtf[i], y = ytf[i];
        const double own = values[i * (size_t)ld + col];
        if (x < 0 || x >= gw || y < 0 || y >= gh) {           // the scatter has raised the flag
            out[e] = __builtin_nan("");
            if (counts) counts[e] = 0;
            continue;
        }
        if (c == 0 && grid[(size_t)y * (size_t)gw + (size_t)x] != (int)i) flag[0] = 1;
        int m = 0, nn = 0;                                    // sorted members, NaN members (nan_absent = 0)
        for (int dy = -R; dy <= R; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= gh) continue;
            for (int dx = -R; dx <= R; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= gw) continue;
                const int j = grid[(size_t)yy * (size_t)gw + (size_t)xx];
                if (j < 0) continue;
                const double v = values[(size_t)j * (size_t)ld + col];
                if (v != v) {
                    if (!nan_absent) ++nn;
                    continue;
                }
                int p = m;                                    // m < M: at most one row per cell
                while (p > 0 && mine[(p - 1) * T] > v) { mine[p * T] = mine[(p - 1) * T]; --p; }
                mine[p * T] = v;
                ++m;
            }
        }
        const int cnt = m + nn;
        double res = own;
        if (nan_absent && own != own) {
            res = __builtin_nan("");
        } else if (2 * cnt > M) {
            if (nn) res = __builtin_nan("");
            else if (cnt & 1) res = 0.0 + mine[(cnt >> 1) * T];                              // np.mean of one value: 0.0 + a, over 1
            else res = ((0.0 + mine[((cnt >> 1) - 1) * T]) + mine[(cnt >> 1) * T]) / 2.0;
        }
        out[e] = res;
        if (counts) counts[e] = cnt;
    }
}

// ------------------------------------------------------------------------------------------
// 4. number of distinct values of a column
// ------------------------------------------------------------------------------------------
// grid (C, chunks): the block of chunk k holds its sorted keys in registers (CS_CHUNK / 256 per thread), marks the first
// of every run of equal keys, and strikes those that an earlier chunk holds.
__global__ __launch_bounds__(GT_UQ_COUNT_THREADS) void gt_unique_count_kernel(const double* __restrict__ sorted, int npad, int chunks,
                                                                              const int32_t* __restrict__ valid, int32_t* __restrict__ partial) {
    constexpr int Q = CS_CHUNK / GT_UQ_COUNT_THREADS;
    __shared__ double key[CS_CHUNK];
    __shared__ int total;
    const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const double* const col = sorted + (size_t)c * (size_t)npad;
    const int32_t* const vl = valid + (size_t)c * (size_t)chunks;
    const int len = vl[k];
    double x[Q];
    unsigned alive = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int p = q * GT_UQ_COUNT_THREADS + tid;
        x[q] = 0.0;
        if (p < len) {
            x[q] = col[(size_t)k * CS_CHUNK + p];
            if (p == 0 || col[(size_t)k * CS_CHUNK + p - 1] != x[q]) alive |= 1u << q;
        }
    }
    if (tid == 0) total = 0;
    for (int e = 0; e < k; ++e) {
        const int elen = vl[e];
        __syncthreads();                                      // the previous chunk's searches are done
        for (int i = tid; i < elen; i += GT_UQ_COUNT_THREADS) key[i] = col[(size_t)e * CS_CHUNK + i];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (!(alive & (1u << q))) continue;
            const int lo = cs_first_ge(key, elen, x[q]);
            if (lo < elen && key[lo] == x[q]) alive &= ~(1u << q);
        }
    }
    __syncthreads();
    if (alive) atomicAdd(&total, __popc(alive));              // an integer counter in LDS
    __syncthreads();
    if (tid == 0) partial[(size_t)c * (size_t)chunks + k] = total;
}

__global__ __launch_bounds__(256) void gt_unique_finish_kernel(const int32_t* __restrict__ partial, const int32_t* __restrict__ nan_flag, int C,
                                                               int chunks, int32_t* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int s = nan_flag[c] ? 1 : 0;                              // all NaNs together are one value
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)c * (size_t)chunks + k];
    out[c] = s;
}

struct UqPlan {
    int chunks, npad;
    size_t off_valid, off_partial, off_flag, bytes;
};

UqPlan uq_plan(int n, int C) {
    UqPlan p;
    p.chunks = cs_chunks(n);
    p.npad = p.chunks * CS_CHUNK;
    size_t o = sq_align_up((size_t)C * (size_t)p.npad * 8, 256);
    p.off_valid = o;   o += sq_align_up((size_t)C * (size_t)p.chunks * 4, 256);
    p.off_partial = o; o += sq_align_up((size_t)C * (size_t)p.chunks * 4, 256);
    p.off_flag = o;    o += sq_align_up((size_t)C * 4, 256);
    p.bytes = o;
    return p;
}

}  // namespace

static_assert(GT_SPOT_CHUNK * sizeof(double2) <= 32768, "a chunk of spots fits half the static LDS limit");
static_assert((2 * SQ_GT_MAX_RADIUS + 1) * (2 * SQ_GT_MAX_RADIUS + 1) * GT_MF_THREADS * sizeof(double) <= 65536, "the widest window's values fit LDS");
static_assert(CS_CHUNK % GT_UQ_COUNT_THREADS == 0 && CS_CHUNK / GT_UQ_COUNT_THREADS <= 32, "a thread's keys fit its bit mask");
static_assert(SQ_GT_MAX_K == 8, "the mean's pairwise form and the launch table are written for k <= 8");

extern "C" int sq_gt_spot_chunk(void) { return GT_SPOT_CHUNK; }
extern "C" int sq_gt_unique_chunk_rows(void) { return CS_CHUNK; }

extern "C" int sq_gt_nearest_spots(const double* xc, const double* yc, int n_tiles, const double* sx, const double* sy, int n_spots, int k,
                                   int32_t* idx, double* dist, sq_stream_t stream_) {
    SQ_REQUIRE(n_tiles >= 1 && n_tiles <= SQ_MAP_MAX_ROWS, "gt_nearest_spots: n_tiles = %d, must be in 1..%d", n_tiles, SQ_MAP_MAX_ROWS);
    SQ_REQUIRE(n_spots >= 1 && n_spots <= SQ_GT_MAX_SPOTS, "gt_nearest_spots: n_spots = %d, must be in 1..%d", n_spots, SQ_GT_MAX_SPOTS);
    SQ_REQUIRE(k >= 1 && k <= SQ_GT_MAX_K, "gt_nearest_spots: k = %d, must be in 1..%d", k, SQ_GT_MAX_K);
    SQ_REQUIRE(xc && yc && sx && sy && idx, "gt_nearest_spots: null xc, yc, sx, sy or idx pointer");
    SQ_REQUIRE((((uintptr_t)xc | (uintptr_t)yc | (uintptr_t)sx | (uintptr_t)sy | (uintptr_t)dist) & 7) == 0 && ((uintptr_t)idx & 3) == 0,
               "gt_nearest_spots: misaligned pointer");
    const int k_eff = k < n_spots ? k : n_spots;
    hipStream_t st = (hipStream_t)stream_;
    switch (k) {
        case 1: gt_launch_nearest<1>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 2: gt_launch_nearest<2>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 3: gt_launch_nearest<3>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 4: gt_launch_nearest<4>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 5: gt_launch_nearest<5>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 6: gt_launch_nearest<6>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        case 7: gt_launch_nearest<7>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
        default: gt_launch_nearest<8>(xc, yc, n_tiles, sx, sy, n_spots, k_eff, idx, dist, st); break;
    }
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" int sq_gt_spot_means(const int32_t* idx, int n_tiles, int k_eff, const void* expr, int expr_f64, int n_spots, int ld,
                                const int32_t* cols, int C, double* out, sq_stream_t stream_) {
    SQ_REQUIRE(n_tiles >= 1 && n_tiles <= SQ_MAP_MAX_ROWS, "gt_spot_means: n_tiles = %d, must be in 1..%d", n_tiles, SQ_MAP_MAX_ROWS);
    SQ_REQUIRE(n_spots >= 1 && n_spots <= SQ_GT_MAX_SPOTS, "gt_spot_means: n_spots = %d, must be in 1..%d", n_spots, SQ_GT_MAX_SPOTS);
    SQ_REQUIRE(k_eff >= 1 && k_eff <= SQ_GT_MAX_K && k_eff <= n_spots, "gt_spot_means: k_eff = %d, must be in 1..min(%d, n_spots = %d)", k_eff,
               SQ_GT_MAX_K, n_spots);
    SQ_REQUIRE_COLUMNS("gt_spot_means", "C", C, 0, ld, cols);
    SQ_REQUIRE(expr_f64 == 0 || expr_f64 == 1, "gt_spot_means: expr_f64 = %d, must be 0 (f32) or 1 (f64)", expr_f64);
    SQ_REQUIRE(idx && expr && out, "gt_spot_means: null idx, expr or out pointer");
    SQ_REQUIRE(((uintptr_t)expr & (expr_f64 ? 7 : 3)) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)cols & 3) == 0 && ((uintptr_t)idx & 3) == 0,
               "gt_spot_means: misaligned pointer");
    const unsigned blocks = cs_blocks((size_t)n_tiles * (size_t)C, 256);
    hipStream_t st = (hipStream_t)stream_;
    if (expr_f64)
        hipLaunchKernelGGL(gt_spot_means_kernel<double>, dim3(blocks), dim3(256), 0, st, idx, n_tiles, k_eff, (const double*)expr, n_spots, ld, cols,
                           C, out);
    else
        hipLaunchKernelGGL(gt_spot_means_kernel<float>, dim3(blocks), dim3(256), 0, st, idx, n_tiles, k_eff, (const float*)expr, n_spots, ld, cols,
                           C, out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_gt_median_filter_workspace_bytes(int n, int grid_w, int grid_h) {
    if (n < 1 || n > SQ_MAP_MAX_ROWS || grid_w < 1 || grid_h < 1 || (long long)grid_w * (long long)grid_h > SQ_GT_MAX_GRID_CELLS) return 0;
    return sq_align_up((size_t)grid_w * (size_t)grid_h * 4, 256);
}

extern "C" int sq_gt_median_filter(const double* values, int n, int ld, const int32_t* cols, int C, const int32_t* xtf, const int32_t* ytf,
                                   int grid_w, int grid_h, int r, int nan_absent, double* out, int32_t* counts, uint8_t* flag,
                                   void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE_TABLE("gt_median_filter", n, 1, SQ_MAP_MAX_ROWS, "C", C, 0, ld, cols);
    SQ_REQUIRE(grid_w >= 1 && grid_h >= 1 && (long long)grid_w * (long long)grid_h <= SQ_GT_MAX_GRID_CELLS,
               "gt_median_filter: grid %d x %d, both extents must be at least 1 and their product at most %d", grid_w, grid_h, SQ_GT_MAX_GRID_CELLS);
    SQ_REQUIRE(r >= 1 && r <= SQ_GT_MAX_RADIUS, "gt_median_filter: radius r = %d, must be in 1..%d", r, SQ_GT_MAX_RADIUS);
    SQ_REQUIRE(nan_absent == 0 || nan_absent == 1, "gt_median_filter: nan_absent = %d, must be 0 or 1", nan_absent);
    SQ_REQUIRE(values && xtf && ytf && out && flag && workspace, "gt_median_filter: null values, xtf, ytf, out, flag or workspace pointer");
    SQ_REQUIRE((((uintptr_t)values | (uintptr_t)out | (uintptr_t)workspace) & 7) == 0 &&
               (((uintptr_t)cols | (uintptr_t)xtf | (uintptr_t)ytf | (uintptr_t)counts) & 3) == 0, "gt_median_filter: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("gt_median_filter", workspace_bytes, sq_gt_median_filter_workspace_bytes(n, grid_w, grid_h));
    hipStream_t st = (hipStream_t)stream_;
    int32_t* const grid = (int32_t*)workspace;
    SQ_HIP_CHECK(hipMemsetAsync(grid, 0xFF, (size_t)grid_w * (size_t)grid_h * 4, st));          // every cell -1
    hipLaunchKernelGGL(gt_grid_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xtf, ytf, n, grid_w, grid_h, grid, flag);
    SQ_LAUNCH_CHECK();
    const unsigned blocks = cs_blocks((size_t)n * (size_t)C, GT_MF_THREADS);
    if (r == 1)
        hipLaunchKernelGGL(gt_median_kernel<1>, dim3(blocks), dim3(GT_MF_THREADS), 0, st, values, n, ld, cols, C, xtf, ytf, grid_w, grid_h,
                           (const int32_t*)grid, nan_absent, out, counts, flag);
    else if (r == 2)
        hipLaunchKernelGGL(gt_median_kernel<2>, dim3(blocks), dim3(GT_MF_THREADS), 0, st, values, n, ld, cols, C, xtf, ytf, grid_w, grid_h,
                           (const int32_t*)grid, nan_absent, out, counts, flag);
    else
        hipLaunchKernelGGL(gt_median_kernel<3>, dim3(blocks), dim3(GT_MF_THREADS), 0, st, values, n, ld, cols, C, xtf, ytf, grid_w, grid_h,
                           (const int32_t*)grid, nan_absent, out, counts, flag);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_gt_count_unique_workspace_bytes(int n, int C) {
    if (n < 1 || n > SQ_MAP_MAX_ROWS || C < 1 || C > SQ_GT_MAX_UNIQUE_COLS) return 0;
    return uq_plan(n, C).bytes;
}

extern "C" int sq_gt_count_unique(const double* values, int n, int ld, const int32_t* cols, int C, int32_t* out, void* workspace,
                                  size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE_TABLE("gt_count_unique", n, 1, SQ_MAP_MAX_ROWS, "C", C, SQ_GT_MAX_UNIQUE_COLS, ld, cols);
    SQ_REQUIRE(values && out && workspace, "gt_count_unique: null values, out or workspace pointer");
    SQ_REQUIRE((((uintptr_t)values | (uintptr_t)workspace) & 7) == 0 && (((uintptr_t)cols | (uintptr_t)out) & 3) == 0,
               "gt_count_unique: misaligned pointer");
    const UqPlan p = uq_plan(n, C);
    SQ_REQUIRE_WORKSPACE("gt_count_unique", workspace_bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream_;
    char* const ws = (char*)workspace;
    double* const sorted = (double*)ws;
    int32_t* const valid = (int32_t*)(ws + p.off_valid);
    int32_t* const partial = (int32_t*)(ws + p.off_partial);
    int32_t* const nan_flag = (int32_t*)(ws + p.off_flag);
    if (int e = cs_sort_chunks(values, 1, n, ld, cols, C, sorted, valid, nan_flag, st)) return e;
    hipLaunchKernelGGL(gt_unique_count_kernel, dim3((unsigned)C, (unsigned)p.chunks), dim3(GT_UQ_COUNT_THREADS), 0, st, (const double*)sorted,
                       p.npad, p.chunks, (const int32_t*)valid, partial);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(gt_unique_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const int32_t*)partial,
                       (const int32_t*)nan_flag, C, p.chunks, out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
