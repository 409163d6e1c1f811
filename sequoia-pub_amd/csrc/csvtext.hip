// The spatial prediction table as CSV text on the device (include/sequoia_hip.h, "CSV text"): the fold mean of
// spatial_vis/visualize.py:299-300 and the bytes DataFrame.to_csv writes for the rows of an int64 index, int64 columns and
// float32 columns.  fmt_core.h holds the text of a cell as host-and-device functions; this file lays the cells out.
//   fold mean  one thread per (row, column): the folds added in order in fp32 from +0.0, a NaN counting as +0.0, the sum
//              divided (correctly rounded) by the fp32 count of values that are not NaN; no such value: NaN.  That is
//              pandas' nanmean on float32 columns bit for bit (-0.0 alone gives +0.0, as there).
//   format     the rows of a call are ONE flat array of cells (row-major: index, ints, floats), CT_TILE cells per
//              workgroup, CT_ITEMS consecutive cells per thread -- a row of 10^5 cells is a hundred workgroups' work:
//              1. ct_len_kernel    the length of every cell with its ',' or '\n' (uint8) and the sum per workgroup;
//              2. ct_scan_kernel   one workgroup: exclusive scan of those sums (int64), the total, the overflow status;
//              3. ct_write_kernel  scan of the tile's lengths, every thread writes its cells into an LDS image of the tile's
//                                  text (at most CT_TILE * SQF_MAX_CELL bytes), the workgroup stores the image as dwords.
//              A cell is formatted twice (length, bytes) instead of keeping nine digits and an exponent per cell.
// Offsets are 64-bit; a byte is stored only if it lies below `capacity`; no workgroup waits for another (three launches
// in stream order); every loop is bounded by the tile, the segment of the scan or fmt_core.h's constants.
#include "sq_common.h"
#include "fmt_core.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_ITEMS = 4;
constexpr int CT_TILE = CT_THREADS * CT_ITEMS;
constexpr int CT_SCAN_THREADS = 1024;
constexpr int CT_MEAN_THREADS = 256;

// exclusive scan of one value per thread over the workgroup (CT_THREADS = 4 waves); total: the workgroup's sum
__device__ __forceinline__ uint32_t ct_block_scan(uint32_t v, uint32_t* wave_total, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t below = __shfl_up(inc, o, 64);
        if (lane >= o) inc += below;
    }
    if (lane == 63) wave_total[w] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < CT_THREADS / 64; ++k) {
        if (k < w) before += wave_total[k];
        total += wave_total[k];
    }
    return before + inc - v;
}

__global__ __launch_bounds__(CT_THREADS) void ct_len_kernel(SqfTable t, long long row0, long long cells, int C, uint8_t* __restrict__ len,
                                                            uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_total[CT_THREADS / 64];
    const long long first = (long long)blockIdx.x * CT_TILE + (long long)threadIdx.x * CT_ITEMS;
    long long r = first / C;
    int j = (int)(first - r * C);
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < CT_ITEMS; ++k) {
        if (first + k < cells) {
            const int l = sqf_cell<false>(t, row0 + r, j, nullptr);
            len[first + k] = (uint8_t)l;
            mine += (uint32_t)l;
        }
        if (++j == C) {
            j = 0;
            ++r;
        }
    }
    uint32_t total;
    ct_block_scan(mine, wave_total, total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// thread i owns the sums [i * seg, (i + 1) * seg): its partial, thread 0 adds the CT_SCAN_THREADS partials in order, then
// every thread lays its segment out
__global__ __launch_bounds__(CT_SCAN_THREADS) void ct_scan_kernel(const uint32_t* __restrict__ block_sum, int nb, int seg, long long capacity,
                                                                  int64_t* __restrict__ block_off, int64_t* __restrict__ total,
                                                                  int32_t* __restrict__ status, int64_t* __restrict__ last_row_offset) {
    __shared__ long long part[CT_SCAN_THREADS];
    const int lo = threadIdx.x * seg < nb ? threadIdx.x * seg : nb;
    const int hi = lo + seg < nb ? lo + seg : nb;
    long long mine = 0;
    for (int b = lo; b < hi; ++b) mine += block_sum[b];
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < CT_SCAN_THREADS; ++i) {
            const long long p = part[i];
            part[i] = run;
            run += p;
        }
        total[0] = run;
        last_row_offset[0] = run;
        status[0] = run > capacity ? SQ_CSV_OVERFLOW : SQ_CSV_OK;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (int b = lo; b < hi; ++b) {
        block_off[b] = run;
        run += block_sum[b];
    }
}

__global__ __launch_bounds__(CT_THREADS) void ct_write_kernel(SqfTable t, long long row0, long long cells, int C, const uint8_t* __restrict__ len,
                                                              const int64_t* __restrict__ block_off, uint8_t* __restrict__ out, long long capacity,
                                                              int64_t* __restrict__ row_offsets) {
    __shared__ uint32_t wave_total[CT_THREADS / 64];
    __shared__ __attribute__((aligned(4))) char text[CT_TILE * SQF_MAX_CELL];
    const long long first = (long long)blockIdx.x * CT_TILE + (long long)threadIdx.x * CT_ITEMS;
    uint32_t l[CT_ITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < CT_ITEMS; ++k) {
        l[k] = first + k < cells ? len[first + k] : 0u;
        mine += l[k];
    }
    uint32_t bytes;                                              // of the tile: at most CT_TILE * SQF_MAX_CELL
    uint32_t at = ct_block_scan(mine, wave_total, bytes);
    const long long g0 = block_off[blockIdx.x];
    long long r = first / C;
    int j = (int)(first - r * C);
#pragma unroll
    for (int k = 0; k < CT_ITEMS; ++k) {
        if (first + k < cells) {
            if (j == 0) row_offsets[r] = g0 + at;
            if (at + l[k] <= (uint32_t)sizeof(text)) sqf_cell<true>(t, row0 + r, j, text + at);      // (holds: l is pass 1's length of this cell)
            at += l[k];
        }
        if (++j == C) {
            j = 0;
            ++r;
        }
    }
    __syncthreads();
    // the image to out[g0 .. g0 + bytes): single bytes up to the first 4-byte boundary of `out`, dwords, single bytes
    const uint32_t head = min(bytes, (uint32_t)((4 - (g0 & 3)) & 3));
    const uint32_t words = (bytes - head) >> 2;
    if (threadIdx.x < head && g0 + threadIdx.x < capacity) out[g0 + threadIdx.x] = (uint8_t)text[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < words; w += CT_THREADS) {
        const uint32_t p = head + 4u * w;
        if (g0 + p + 4 <= capacity) {
            const uint32_t v = (uint32_t)(uint8_t)text[p] | (uint32_t)(uint8_t)text[p + 1] << 8 | (uint32_t)(uint8_t)text[p + 2] << 16 |
                               (uint32_t)(uint8_t)text[p + 3] << 24;
            *(uint32_t*)(out + g0 + p) = v;
        } else {
            for (uint32_t q = p; q < p + 4u; ++q)
                if (g0 + q < capacity) out[g0 + q] = (uint8_t)text[q];
        }
    }
    const uint32_t tail = head + 4u * words + threadIdx.x;
    if (tail < bytes && g0 + tail < capacity) out[g0 + tail] = (uint8_t)text[tail];
}

__global__ __launch_bounds__(CT_MEAN_THREADS) void ct_fold_mean_kernel(const float* __restrict__ x, int F, long long fold_stride, long long n, int cols,
                                                                       long long ld, float* __restrict__ out, long long ld_out) {
    const long long cells = n * cols;
    for (long long e = (long long)blockIdx.x * CT_MEAN_THREADS + threadIdx.x; e < cells; e += (long long)gridDim.x * CT_MEAN_THREADS) {
        const long long r = e / cols;
        const int c = (int)(e - r * cols);
        const float* p = x + r * ld + c;
        float sum = 0.0f;
        int count = 0;
        for (int f = 0; f < F; ++f) {
            const float v = p[f * fold_stride];
            const bool is_nan = v != v;
            sum = sum + (is_nan ? 0.0f : v);
            count += is_nan ? 0 : 1;
        }
        out[r * ld_out + c] = count ? __fdiv_rn(sum, (float)count) : __builtin_nanf("");
    }
}

struct CtPlan {
    long long rows, cells;
    int C, nb, seg;
    size_t len_bytes, sum_bytes, off_bytes;
};

bool ct_plan(long long rows, int n_int, int n_f32, CtPlan* p) {
    if (rows < 1 || n_int < 0 || n_f32 < 0 || n_int > SQ_CSV_MAX_COLUMNS || n_f32 > SQ_CSV_MAX_COLUMNS) return false;
    p->rows = rows;
    p->C = 1 + n_int + n_f32;
    if (rows > SQ_CSV_MAX_CELLS / p->C) return false;
    p->cells = rows * p->C;
    p->nb = (int)((p->cells + CT_TILE - 1) / CT_TILE);
    p->seg = (p->nb + CT_SCAN_THREADS - 1) / CT_SCAN_THREADS;
    p->len_bytes = sq_align_up((size_t)p->cells, 256);
    p->sum_bytes = sq_align_up((size_t)p->nb * 4, 256);
    p->off_bytes = sq_align_up((size_t)p->nb * 8, 256);
    return true;
}

}  // namespace

static_assert(SQF_MAX_CELL == SQ_CSV_MAX_CELL_BYTES && SQF_MAX_CELL < 256, "a cell's length fits the uint8 of pass 1");
static_assert(CT_TILE * SQF_MAX_CELL <= 32768, "the text image of a tile and the wave totals fit 64 KB of LDS twice over");
static_assert((long long)SQ_CSV_MAX_CELLS / CT_TILE / CT_SCAN_THREADS <= 1024, "a scan thread owns at most 1024 sums");

extern "C" int sq_fold_mean_f32(const float* x, int n_folds, long long fold_stride, long long n, int cols, long long ld, float* out,
                                long long ld_out, sq_stream_t stream_) {
    SQ_REQUIRE(n_folds >= 1 && n_folds <= SQ_CSV_MAX_FOLDS, "fold_mean_f32: n_folds = %d, must be in 1..%d", n_folds, SQ_CSV_MAX_FOLDS);
    SQ_REQUIRE(n >= 1 && cols >= 1 && cols <= SQ_CSV_MAX_COLUMNS && n <= SQ_CSV_MAX_CELLS / cols,
               "fold_mean_f32: n = %lld rows of %d columns, must be at least 1 x 1, at most %d columns and %d cells", n, cols,
               SQ_CSV_MAX_COLUMNS, SQ_CSV_MAX_CELLS);
    SQ_REQUIRE(ld >= cols && ld_out >= cols && fold_stride >= 0, "fold_mean_f32: ld = %lld, ld_out = %lld for %d columns, fold_stride = %lld", ld,
               ld_out, cols, fold_stride);
    SQ_REQUIRE(x && out, "fold_mean_f32: null x or out pointer");
    SQ_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "fold_mean_f32: misaligned pointer");
    const long long cells = n * cols;
    const long long blocks = (cells + CT_MEAN_THREADS - 1) / CT_MEAN_THREADS;
    hipLaunchKernelGGL(ct_fold_mean_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(CT_MEAN_THREADS), 0, (hipStream_t)stream_, x, n_folds,
                       fold_stride, n, cols, ld, out, ld_out);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_csv_format_workspace_bytes(long long rows, int n_int, int n_f32) {
    CtPlan p;
    if (!ct_plan(rows, n_int, n_f32, &p)) {
        sq_set_error("csv_format_rows: %lld rows of 1 + %d + %d cells, must be at least 1 row, at most %d columns of a kind and %d cells", rows, n_int,
                     n_f32, SQ_CSV_MAX_COLUMNS, SQ_CSV_MAX_CELLS);
        return 0;
    }
    return p.len_bytes + p.sum_bytes + p.off_bytes;
}

extern "C" int sq_csv_format_rows(const int64_t* index, const int64_t* ints, int n_int, const float* f32, int n_f32, long long ld_f32,
                                  long long row_lo, long long row_hi, uint8_t* out, long long capacity, int64_t* row_offsets, int64_t* total,
                                  int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    CtPlan p;
    SQ_REQUIRE(row_lo >= 0 && row_hi > row_lo, "csv_format_rows: rows %lld..%lld, must be a non-empty range from 0 on", row_lo, row_hi);
    const size_t need = sq_csv_format_workspace_bytes(row_hi - row_lo, n_int, n_f32);
    if (need == 0 || !ct_plan(row_hi - row_lo, n_int, n_f32, &p)) return SQ_ERR_ARG;
    SQ_REQUIRE(ld_f32 >= n_f32, "csv_format_rows: ld_f32 = %lld for n_f32 = %d columns", ld_f32, n_f32);
    SQ_REQUIRE(capacity >= 0, "csv_format_rows: capacity = %lld", capacity);
    SQ_REQUIRE(index && (ints || n_int == 0) && (f32 || n_f32 == 0) && (out || capacity == 0) && row_offsets && total && status && workspace,
               "csv_format_rows: null pointer");
    SQ_REQUIRE((((uintptr_t)index | (uintptr_t)ints | (uintptr_t)row_offsets | (uintptr_t)total | (uintptr_t)workspace) & 7) == 0 &&
                   (((uintptr_t)f32 | (uintptr_t)out | (uintptr_t)status) & 3) == 0,
               "csv_format_rows: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("csv_format_rows", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream_;
    uint8_t* const len = (uint8_t*)workspace;
    uint32_t* const block_sum = (uint32_t*)(len + p.len_bytes);
    int64_t* const block_off = (int64_t*)((char*)block_sum + p.sum_bytes);
    const SqfTable t = {index, ints, f32, n_int, n_f32, ld_f32};
    SqProf prof(st);
    if (prof.on()) prof.begin("csv_format_rows", 0.0, (double)p.cells * 8.0);
    hipLaunchKernelGGL(ct_len_kernel, dim3((unsigned)p.nb), dim3(CT_THREADS), 0, st, t, row_lo, p.cells, p.C, len, block_sum);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_scan_kernel, dim3(1), dim3(CT_SCAN_THREADS), 0, st, (const uint32_t*)block_sum, p.nb, p.seg, capacity, block_off, total, status,
                       row_offsets + p.rows);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_write_kernel, dim3((unsigned)p.nb), dim3(CT_THREADS), 0, st, t, row_lo, p.cells, p.C, (const uint8_t*)len,
                       (const int64_t*)block_off, out, capacity, row_offsets);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
