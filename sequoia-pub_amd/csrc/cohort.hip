// Device-resident cohort feed: one batch of a cohort's cluster features and targets, gathered from tables that stay on the device.
//   /root/reference/src/read_data.py:38-56   __getitem__: one HDF5 open and read per slide and epoch
//   /root/reference/src/utils.py:10-18       custom_collate_fn: default_collate's stack of the readable items
//   /root/reference/src/main.py:112-135      the DataLoaders (pinned copy, upload) of the three roles of every fold
// With the tables loaded once (sequoia-pub_amd/data.py: CohortTable) a batch is rows index[0..m) of both tables: sq_cohort_gather.
#include "sq_common.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_UNROLL = 4;                           // units per thread and tile: all loads of a tile are issued before its stores
constexpr int CG_TILE = CG_THREADS * CG_UNROLL;        // units per tile
constexpr int CG_MAX_BLOCKS = 2048;                    // 256 CUs x 8 blocks; the rest is grid-strided

struct CgArgs {
    const float* x_table;
    const float* y_table;   // null: features only (units_y = 0)
    float* x_out;
    float* y_out;
    const int32_t* index;   // [m] or null for the identity
    int n_slides, m;
    long long row_x, row_y;       // floats per row
    long long units_x, units_y;   // units per row: 16-byte units where the table's rows are moved as vectors, dwords otherwise
    long long chunks, tiles;      // tiles per output row, tiles in all = m * chunks
};

// Output row j = table row index[j]; a row of both tables is cut into units_x + units_y units and a tile is CG_TILE consecutive
// units of one row.  VX / VY: the unit of that table is 16 bytes (every row of the table AND of the output starts on 16 bytes: the
// launcher decides that from the row length and the two base pointers), else a dword -- so a vector row never has a tail.
// Every offset into a table is 64-bit: row index[j] of a [7584, 100, 1024] table starts beyond 2^31 bytes from row 5243 on.
template <bool VX, bool VY>
__global__ __launch_bounds__(CG_THREADS) void cohort_gather_kernel(const CgArgs a) {
    for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const long long j = t / a.chunks;
        const long long u0 = (t - j * a.chunks) * CG_TILE + threadIdx.x;
        // an index outside [0, n_slides) is compared before any address is formed from it and gives zero rows
        const int from = a.index ? a.index[j] : (int)j;
        const bool live = from >= 0 && from < a.n_slides;
        const float* const xs = a.x_table + (size_t)(live ? from : 0) * (size_t)a.row_x;
        const float* const ys = a.y_table + (size_t)(live ? from : 0) * (size_t)a.row_y;      // never read when units_y = 0
        float* const xd = a.x_out + (size_t)j * (size_t)a.row_x;
        float* const yd = a.y_out + (size_t)j * (size_t)a.row_y;
        f32x4 v[CG_UNROLL];
#pragma unroll
        for (int k = 0; k < CG_UNROLL; ++k) {
            const long long u = u0 + (long long)k * CG_THREADS;
            v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!live) continue;
            if (u < a.units_x) {
                if constexpr (VX) v[k] = *(const f32x4*)(xs + 4 * u);
                else v[k][0] = xs[u];
            } else if (u < a.units_x + a.units_y) {
                const long long w = u - a.units_x;
                if constexpr (VY) v[k] = *(const f32x4*)(ys + 4 * w);
                else v[k][0] = ys[w];
            }
        }
#pragma unroll
        for (int k = 0; k < CG_UNROLL; ++k) {
            const long long u = u0 + (long long)k * CG_THREADS;
            if (u < a.units_x) {
                if constexpr (VX) *(f32x4*)(xd + 4 * u) = v[k];
                else xd[u] = v[k][0];
            } else if (u < a.units_x + a.units_y) {
                const long long w = u - a.units_x;
                if constexpr (VY) *(f32x4*)(yd + 4 * w) = v[k];
                else yd[w] = v[k][0];
            }
        }
    }
}

// every row of `table` and of `out` starts 16-byte aligned
bool cg_rows_on_16(const float* table, const float* out, long long row) {
    return row % 4 == 0 && (((uintptr_t)table | (uintptr_t)out) & 15) == 0;
}

}  // namespace

extern "C" int sq_cohort_gather(const float* x_table, const float* y_table, int n_slides, long long row_x, long long row_y,
                                const int32_t* index, int m, float* x_out, float* y_out, sq_stream_t stream_) {
    SQ_REQUIRE(m >= 0 && n_slides >= 0, "cohort_gather: m = %d output rows from n_slides = %d", m, n_slides);
    SQ_REQUIRE(index || m == n_slides, "cohort_gather: a null index is the identity and takes m = n_slides, got m = %d, n_slides = %d", m,
               n_slides);
    SQ_REQUIRE(((uintptr_t)index & 3) == 0, "cohort_gather: misaligned index (int32)");
    SQ_REQUIRE((y_table == nullptr) == (y_out == nullptr),
               "cohort_gather: y_table and y_out are given together or both null (a features-only gather), got one of them");
    const bool with_y = y_table != nullptr;
    SQ_REQUIRE(row_x >= 1 && row_x <= (1ll << 40), "cohort_gather: row_x = %lld floats per feature row, must be in 1..2^40", row_x);
    SQ_REQUIRE(!with_y || (row_y >= 1 && row_y <= (1ll << 40)), "cohort_gather: row_y = %lld floats per target row, must be in 1..2^40", row_y);
    if (m == 0) return SQ_OK;
    SQ_REQUIRE(n_slides >= 1, "cohort_gather: n_slides = %d table rows for m = %d output rows", n_slides, m);
    SQ_REQUIRE(x_table && x_out, "cohort_gather: null x_table or x_out");
    SQ_REQUIRE((((uintptr_t)x_table | (uintptr_t)x_out | (uintptr_t)y_table | (uintptr_t)y_out) & 3) == 0,
               "cohort_gather: misaligned table or output (float32)");
    CgArgs a;
    a.x_table = x_table; a.y_table = y_table; a.x_out = x_out; a.y_out = y_out; a.index = index;
    a.n_slides = n_slides; a.m = m;
    a.row_x = row_x; a.row_y = with_y ? row_y : 0;
    const bool vx = cg_rows_on_16(x_table, x_out, a.row_x), vy = with_y && cg_rows_on_16(y_table, y_out, a.row_y);
    a.units_x = vx ? a.row_x / 4 : a.row_x;
    a.units_y = vy ? a.row_y / 4 : a.row_y;
    a.chunks = (a.units_x + a.units_y + CG_TILE - 1) / CG_TILE;
    a.tiles = a.chunks * m;                            // <= 2^31 * 2^32
    const dim3 grid((unsigned)(a.tiles < CG_MAX_BLOCKS ? a.tiles : CG_MAX_BLOCKS));
    const hipStream_t st = (hipStream_t)stream_;
    if (vx && vy) hipLaunchKernelGGL((cohort_gather_kernel<true, true>), grid, dim3(CG_THREADS), 0, st, a);
    else if (vx) hipLaunchKernelGGL((cohort_gather_kernel<true, false>), grid, dim3(CG_THREADS), 0, st, a);
    else if (vy) hipLaunchKernelGGL((cohort_gather_kernel<false, true>), grid, dim3(CG_THREADS), 0, st, a);
    else hipLaunchKernelGGL((cohort_gather_kernel<false, false>), grid, dim3(CG_THREADS), 0, st, a);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
