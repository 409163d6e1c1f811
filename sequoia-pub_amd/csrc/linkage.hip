// Average-linkage clustering of the rows of a matrix on the device (include/sequoia_hip.h, "Map statistics"): what
// sns.clustermap(corrdf) of spatial_vis/gbm_celltype_analysis.py:81,145 computes before it draws --
// scipy.cluster.hierarchy.linkage(A, method='average', metric='euclidean') and the leaf order of its dendrogram.
//   row distances  pdist(A, 'euclidean') as scipy's C loop: s = s + d * d over the features in ascending order, the product
//                  and the sum rounded separately (contraction is off for this file), then sqrt.  The order in t is fixed per
//                  pair; the parallelism is across pairs: a workgroup owns a 64 x 64 block of pairs on or above the diagonal,
//                  a thread a 4 x 4 register tile of them, and the two row tiles pass through LDS 32 features at a time
//                  ([t][row], so a wave's reads are a broadcast and a run of neighbours).  The block leaves through LDS, so
//                  both [i][j] and [j][i] are written in rows.  A distance that is not finite raises the problem's status
//                  (an integer atomic max of K - i: the smallest row wins).
//   linkage        scipy's nn_chain for 'average', ONE WORKGROUP PER PROBLEM (as emd.hip): the chain and the cluster sizes in
//                  LDS, the distance matrix in global memory (one coalesced row read per nearest-neighbour search; a merge
//                  reads two rows and writes one row and one column).  A search is a min-reduction over (distance, index)
//                  with scipy's tie rule.  A search checks the row it reads: a live distance that is NaN, infinite or negative
//                  enters the reduction as -inf, wins it, and ends the problem with a status before any index derived from
//                  it is used -- the kernel is safe on a matrix nobody has checked (dist_status = NULL).  Every thread follows
//                  the same control flow from the same reduced values, so the chain's top and the element below it live in
//                  registers.  Then the K - 1 merges are sorted by (distance,
//                  merge number) in LDS (bitonic; the key makes it stable), relabelled by one thread with a union-find whose
//                  parents are in LDS (path halving), and the leaves are that thread's depth-first walk.
// No floating-point atomics and no order that depends on scheduling: two calls give the same bytes.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"

#pragma clang fp contract(off)      // s + d * d and (na * da + nb * db) / (na + nb) are separately rounded operations

namespace {

constexpr double LK_DBL_MAX = 1.7976931348623157e308;     // the largest finite distance

// ------------------------------------------------------------------------------------------
// 1. row distances
// ------------------------------------------------------------------------------------------
constexpr int RD_TILE = 64;               // pairs block: 64 x 64, 256 threads x (4 x 4)
constexpr int RD_KC = 32;                 // features per LDS chunk

// grid (T, T, B), blocks with bx >= by.  worst[b] (zeroed by the entry) ends as K - i for the smallest row i that has a
// distance to another row that is not finite, 0 if there is none.
__global__ __launch_bounds__(256) void row_dist_kernel(const double* __restrict__ a, int K, int M, int ld, double* __restrict__ dist,
                                                       int32_t* __restrict__ worst) {
    if (blockIdx.x < blockIdx.y) return;
    __shared__ double lds[2][RD_KC][RD_TILE + 2];
    const bool diag = blockIdx.x == blockIdx.y;
    const int i0 = blockIdx.y * RD_TILE, j0 = blockIdx.x * RD_TILE;
    const double* const A = a + (size_t)blockIdx.z * (size_t)K * (size_t)ld;
    double* const D = dist + (size_t)blockIdx.z * (size_t)K * (size_t)K;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const double (*const sa)[RD_TILE + 2] = lds[0];
    const double (*const sb)[RD_TILE + 2] = diag ? lds[0] : lds[1];
    double s[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[r][c] = 0.0;
    for (int t0 = 0; t0 < M; t0 += RD_KC) {
        // a thread loads feature t of rows row, row + 8, ...: a wave reads two runs of 32 neighbouring features.  Features past M
        // and rows past K are zeros: d = 0 and s + 0 * 0 leaves s as it is.
#pragma unroll
        for (int p = 0; p < RD_TILE * RD_KC / 256; ++p) {
            const int t = tid & (RD_KC - 1), row = (tid >> 5) + 8 * p;
            const bool t_in = t0 + t < M;
            lds[0][t][row] = t_in && i0 + row < K ? A[(size_t)(i0 + row) * (size_t)ld + (size_t)(t0 + t)] : 0.0;
            if (!diag) lds[1][t][row] = t_in && j0 + row < K ? A[(size_t)(j0 + row) * (size_t)ld + (size_t)(t0 + t)] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < RD_KC; ++t) {
            double ai[4], bj[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ai[r] = sa[t][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) bj[c] = sb[t][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = ai[r] - bj[c];
                    s[r][c] = s[r][c] + d * d;
                }
        }
        __syncthreads();
    }
    // the block through LDS (the chunks are done with it): tile[ii][jj] is the distance of rows i0 + ii and j0 + jj
    static_assert(sizeof(double) * RD_TILE * (RD_TILE + 1) <= sizeof(lds), "the output block fits the staging buffer");
    double (*const tile)[RD_TILE + 1] = reinterpret_cast<double (*)[RD_TILE + 1]>(&lds[0][0][0]);
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ii = ty + 16 * r, jj = tx + 16 * c, gi = i0 + ii, gj = j0 + jj;
            double v = sqrt(s[r][c]);
            if (gi == gj) v = 0.0;
            else if (gi < K && gj < K && !(fabs(v) <= LK_DBL_MAX)) bad = max(bad, K - min(gi, gj));
            tile[ii][jj] = v;
        }
    if (bad) atomicMax(worst + blockIdx.z, bad);
    __syncthreads();
    const int jj = tid & 63;
    for (int ii = tid >> 6; ii < RD_TILE; ii += 4) {
        if (i0 + ii < K && j0 + jj < K) D[(size_t)(i0 + ii) * (size_t)K + (size_t)(j0 + jj)] = tile[ii][jj];
        if (!diag && j0 + ii < K && i0 + jj < K) D[(size_t)(j0 + ii) * (size_t)K + (size_t)(i0 + jj)] = tile[jj][ii];
    }
}

// status[b] = 0, or 1 + the smallest row with a distance that is not finite
__global__ __launch_bounds__(256) void row_dist_status_kernel(const int32_t* __restrict__ worst, int B, int K, int32_t* __restrict__ status) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) status[b] = worst[b] ? K - worst[b] + 1 : 0;
}

// ------------------------------------------------------------------------------------------
// 2. average linkage
// ------------------------------------------------------------------------------------------
constexpr int LK_THREADS = 1024;
constexpr int LK_WAVES = LK_THREADS / 64;
constexpr int LK_EPT = SQ_MAP_MAX_LINK_ROWS / LK_THREADS;      // clusters one thread looks at in a search
constexpr int LK_NONE = 0x7fffffff;
// LDS of the workgroup, by phase.  chain: [0, 4 K) chain, [4 K, 8 K) sizes.  sort: [0, 8 P) distances, [8 Kmax, 8 Kmax + 4 P)
// merge numbers.  relabel: [0, 4 (2 K - 1)) parents, the merge numbers' slots now hold a row's two labels packed 16 : 16.
// walk: [0, 4 K) the stack.
constexpr int LK_LDS_BYTES = 12 * SQ_MAP_MAX_LINK_ROWS;

static_assert(SQ_MAP_MAX_LINK_ROWS % LK_THREADS == 0 && (SQ_MAP_MAX_LINK_ROWS & (SQ_MAP_MAX_LINK_ROWS - 1)) == 0, "the sort pads to a power of two within the bound");
static_assert(2 * SQ_MAP_MAX_LINK_ROWS - 1 <= 65536, "a row's two labels pack into 16 bits each");
static_assert(LK_LDS_BYTES + 1024 <= 65536, "one workgroup's static LDS");

// the order of a search: the smaller distance, then the smaller index
__device__ __forceinline__ void lk_take(double& d, int& i, double d2, int i2) {
    if (d2 < d || (d2 == d && i2 < i)) { d = d2; i = i2; }
}

// min over the workgroup; every thread returns with the same (d, i).  Two scratch sets used in turn: one barrier per call.
__device__ __forceinline__ void lk_reduce(double& d, int& i, double (*red_d)[LK_WAVES], int (*red_i)[LK_WAVES], int& turn) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double d2 = __shfl_xor(d, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        lk_take(d, i, d2, i2);
    }
    if ((threadIdx.x & 63) == 0) { red_d[turn][threadIdx.x >> 6] = d; red_i[turn][threadIdx.x >> 6] = i; }
    __syncthreads();
    d = red_d[turn][0];
    i = red_i[turn][0];
#pragma unroll
    for (int w = 1; w < LK_WAVES; ++w) lk_take(d, i, red_d[turn][w], red_i[turn][w]);
    turn ^= 1;
}

// grid (B).  dist is read and written by this workgroup only; a barrier stands between every write and the reads that follow.
__global__ __launch_bounds__(LK_THREADS) void linkage_average_kernel(double* dist, int K, const int32_t* __restrict__ dist_status,
                                                                     double* __restrict__ Z, int32_t* __restrict__ leaves,
                                                                     int32_t* __restrict__ status, int32_t* rec_a, int32_t* rec_b,
                                                                     double* rec_d, int32_t* rec_n) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LK_LDS_BYTES];
    __shared__ double red_d[2][LK_WAVES];
    __shared__ int red_i[2][LK_WAVES];
    const int prob = blockIdx.x, tid = threadIdx.x;
    if (dist_status && dist_status[prob] != 0) {                // the same for the whole workgroup
        if (tid == 0) status[prob] = SQ_LINK_NONFINITE;
        return;
    }
    double* const D = dist + (size_t)prob * (size_t)K * (size_t)K;
    rec_a += (size_t)prob * (size_t)K;
    rec_b += (size_t)prob * (size_t)K;
    rec_d += (size_t)prob * (size_t)K;
    rec_n += (size_t)prob * (size_t)K;
    Z += (size_t)prob * (size_t)(K - 1) * 4;
    leaves += (size_t)prob * (size_t)K;
    const double inf = __builtin_inf();

    // ---- the nearest-neighbour chain.  A thread reads the sizes of its own clusters (tid, tid + 1024, ...) and is the one
    // that writes them; only a merge reads the two sizes of other threads' clusters, behind a barrier.
    int* const chain = reinterpret_cast<int*>(lds);
    int* const size = reinterpret_cast<int*>(lds) + K;
    for (int i = tid; i < K; i += LK_THREADS) size[i] = 1;
    __syncthreads();
    int len = 0, x = -1, p = -1, turn = 0, searches = 0;
    const int most = 3 * (K - 1);
    for (int m = 0; m < K - 1; ++m) {
        if (len == 0) {                                         // the live cluster of smallest index
            double d = inf;
            int i = LK_NONE;
#pragma unroll
            for (int e = 0; e < LK_EPT; ++e) {
                const int c = tid + e * LK_THREADS;
                if (c < K && size[c] > 0) lk_take(d, i, 0.0, c);
            }
            lk_reduce(d, i, red_d, red_i, turn);
            if (i == LK_NONE) {                                 // fewer than two live clusters: not reachable, never an index
                if (tid == 0) status[prob] = SQ_LINK_BAD_DISTANCE;
                return;
            }
            x = i;
            p = -1;
            len = 1;
            if (tid == 0) chain[0] = x;
        }
        double dmin;
        int y;
        for (;;) {
            if (++searches > most) {                            // not reachable by the chain's own argument; no input can spin
                if (tid == 0) status[prob] = SQ_LINK_SEARCH_BOUND;
                return;
            }
            const double* const row = D + (size_t)x * (size_t)K;
            const double dp = len > 1 ? row[p] : inf;           // asked for with the row, not behind the reduction
            double d = inf;
            int i = LK_NONE;
#pragma unroll
            for (int e = 0; e < LK_EPT; ++e) {
                const int c = tid + e * LK_THREADS;
                if (c < K && c != x && size[c] > 0) {
                    const double v = row[c];
                    lk_take(d, i, v >= 0.0 && v <= LK_DBL_MAX ? v : -inf, c);      // a bad distance wins the reduction
                }
            }
            lk_reduce(d, i, red_d, red_i, turn);
            if (i == LK_NONE || d < 0.0) {                      // the same for the whole workgroup; nothing is pushed or merged
                if (tid == 0) status[prob] = SQ_LINK_BAD_DISTANCE;
                return;
            }
            dmin = d;
            y = i;
            if (len > 1 && !(dmin < dp)) y = p;                 // the previous element wins ties
            if (len > 1 && y == p) break;
            if (tid == 0) chain[len] = y;
            ++len;
            p = x;
            x = y;
        }
        // ---- merge x and y: the smaller index dies, the larger carries the cluster
        len -= 2;
        const int ca = min(x, y), cb = max(x, y);
        const int na = size[ca], nb = size[cb];
        const double* const row_a = D + (size_t)ca * (size_t)K;
        double* const row_b = D + (size_t)cb * (size_t)K;
#pragma unroll
        for (int e = 0; e < LK_EPT; ++e) {
            const int c = tid + e * LK_THREADS;
            if (c < K && c != ca && c != cb && size[c] > 0) {
                const double v = ((double)na * row_a[c] + (double)nb * row_b[c]) / (double)(na + nb);
                row_b[c] = v;
                D[(size_t)c * (size_t)K + (size_t)cb] = v;
            }
        }
        if (tid == 0) { rec_a[m] = ca; rec_b[m] = cb; rec_d[m] = dmin; rec_n[m] = na + nb; }
        __syncthreads();                                        // the two sizes are read, the chain's pushes are visible
        if (tid == (ca & (LK_THREADS - 1))) size[ca] = 0;
        if (tid == (cb & (LK_THREADS - 1))) size[cb] = na + nb;
        x = len >= 1 ? chain[len - 1] : -1;
        p = len >= 2 ? chain[len - 2] : -1;
    }
    __syncthreads();

    // ---- sort the merges by (distance, merge number)
    const int n = K - 1;
    int P = 1;
    while (P < n) P <<= 1;
    double* const key_d = reinterpret_cast<double*>(lds);
    int* const key_i = reinterpret_cast<int*>(lds + 8 * SQ_MAP_MAX_LINK_ROWS);
    for (int i = tid; i < P; i += LK_THREADS) {
        key_d[i] = i < n ? rec_d[i] : inf;
        key_i[i] = i < n ? i : LK_NONE;
    }
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < P; i += LK_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const double di = key_d[i], dl = key_d[l];
                    const int ii = key_i[i], il = key_i[l];
                    const bool after = di > dl || (di == dl && ii > il);          // [i] sorts behind [l]
                    if (after == ((i & k) == 0)) { key_d[i] = dl; key_d[l] = di; key_i[i] = il; key_i[l] = ii; }
                }
            }
        }
    __syncthreads();

    // ---- relabel in sorted order: row r's slot takes its two points, then (one thread) the roots of their clusters
    int* const parent = reinterpret_cast<int*>(lds);
    for (int r = tid; r < n; r += LK_THREADS) {
        const int o = key_i[r];
        Z[(size_t)r * 4 + 2] = rec_d[o];
        Z[(size_t)r * 4 + 3] = (double)rec_n[o];
        key_i[r] = rec_a[o] | (rec_b[o] << 16);
    }
    for (int i = tid; i < 2 * K - 1; i += LK_THREADS) parent[i] = i;
    __syncthreads();
    if (tid == 0) {
        for (int r = 0; r < n; ++r) {
            const int packed = key_i[r];
            int ra = packed & 0xffff, rb = packed >> 16;
            while (parent[ra] != ra) { const int g = parent[parent[ra]]; parent[ra] = g; ra = g; }
            while (parent[rb] != rb) { const int g = parent[parent[rb]]; parent[rb] = g; rb = g; }
            key_i[r] = min(ra, rb) | (max(ra, rb) << 16);
            parent[ra] = parent[rb] = K + r;
        }
        // the leaves: depth first from the last row's node, the left child first.  The stack holds disjoint subtrees: at most K.
        int* const stack = reinterpret_cast<int*>(lds);
        int sp = 0, out = 0;
        stack[sp++] = 2 * K - 2;
        for (int visit = 0; visit < 2 * K - 1 && sp > 0; ++visit) {          // a tree of 2K - 1 nodes: the walk cannot run on
            const int node = stack[--sp];
            if (node < K) {
                if (out < K) leaves[out++] = node;
            } else {
                const int packed = key_i[node - K];
                stack[sp++] = packed >> 16;
                stack[sp++] = packed & 0xffff;
            }
        }
        status[prob] = SQ_LINK_OK;
    }
    __syncthreads();
    for (int r = tid; r < n; r += LK_THREADS) {
        const int packed = key_i[r];
        Z[(size_t)r * 4 + 0] = (double)(packed & 0xffff);
        Z[(size_t)r * 4 + 1] = (double)(packed >> 16);
    }
}

bool lk_shape_ok(const char* name, int B, int K) {
    if (K < 2 || K > SQ_MAP_MAX_LINK_ROWS) {
        sq_set_error("%s: K = %d rows, must be in 2..%d", name, K, SQ_MAP_MAX_LINK_ROWS);
        return false;
    }
    if (B < 1 || B > SQ_MAP_MAX_LINK_BATCH) {
        sq_set_error("%s: B = %d problems, must be in 1..%d", name, B, SQ_MAP_MAX_LINK_BATCH);
        return false;
    }
    return true;
}

// workspace of the linkage: the merges as they are made -- per problem K slots of a, b (int32), distance (f64), size (int32)
size_t lk_part(int B, int K, size_t width) { return sq_align_up((size_t)B * (size_t)K * width, 256); }

}  // namespace

extern "C" size_t sq_map_row_distances_workspace_bytes(int B, int K, int M) {
    if (K < 2 || K > SQ_MAP_MAX_LINK_ROWS || B < 1 || B > SQ_MAP_MAX_LINK_BATCH || M < 1 || M > SQ_MAP_MAX_ROWS) return 0;
    return sq_align_up((size_t)B * 4, 256);
}

extern "C" int sq_map_row_distances(const double* a, int B, int K, int M, int ld, double* dist, int32_t* status, void* workspace,
                                    size_t workspace_bytes, sq_stream_t stream_) {
    if (!lk_shape_ok("map_row_distances", B, K)) return SQ_ERR_ARG;
    SQ_REQUIRE(M >= 1 && M <= SQ_MAP_MAX_ROWS, "map_row_distances: M = %d features, must be in 1..%d", M, SQ_MAP_MAX_ROWS);
    SQ_REQUIRE(ld >= M, "map_row_distances: leading dimension ld = %d for M = %d features (M <= ld)", ld, M);
    SQ_REQUIRE(a && dist && status && workspace, "map_row_distances: null a, dist, status or workspace pointer");
    SQ_REQUIRE(((uintptr_t)a & 7) == 0 && ((uintptr_t)dist & 7) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
               "map_row_distances: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("map_row_distances", workspace_bytes, sq_map_row_distances_workspace_bytes(B, K, M));
    hipStream_t st = (hipStream_t)stream_;
    int32_t* const worst = (int32_t*)workspace;
    const unsigned T = (unsigned)((K + RD_TILE - 1) / RD_TILE);
    SQ_HIP_CHECK(hipMemsetAsync(worst, 0, (size_t)B * sizeof(int32_t), st));
    hipLaunchKernelGGL(row_dist_kernel, dim3(T, T, (unsigned)B), dim3(256), 0, st, a, K, M, ld, dist, worst);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_dist_status_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (const int32_t*)worst, B, K, status);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_map_linkage_average_workspace_bytes(int B, int K) {
    if (K < 2 || K > SQ_MAP_MAX_LINK_ROWS || B < 1 || B > SQ_MAP_MAX_LINK_BATCH) return 0;
    return 3 * lk_part(B, K, 4) + lk_part(B, K, 8);
}

extern "C" int sq_map_linkage_average(double* dist, int B, int K, const int32_t* dist_status, double* Z, int32_t* leaves,
                                      int32_t* status, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    if (!lk_shape_ok("map_linkage_average", B, K)) return SQ_ERR_ARG;
    SQ_REQUIRE(dist && Z && leaves && status && workspace, "map_linkage_average: null dist, Z, leaves, status or workspace pointer");
    SQ_REQUIRE(((uintptr_t)dist & 7) == 0 && ((uintptr_t)Z & 7) == 0 && ((uintptr_t)leaves & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
               ((uintptr_t)dist_status & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "map_linkage_average: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("map_linkage_average", workspace_bytes, sq_map_linkage_average_workspace_bytes(B, K));
    char* const ws = (char*)workspace;
    double* const rec_d = (double*)ws;
    int32_t* const rec_a = (int32_t*)(ws + lk_part(B, K, 8));
    int32_t* const rec_b = (int32_t*)(ws + lk_part(B, K, 8) + lk_part(B, K, 4));
    int32_t* const rec_n = (int32_t*)(ws + lk_part(B, K, 8) + 2 * lk_part(B, K, 4));
    hipLaunchKernelGGL(linkage_average_kernel, dim3((unsigned)B), dim3(LK_THREADS), 0, (hipStream_t)stream_, dist, K, dist_status, Z, leaves,
                       status, rec_a, rec_b, rec_d, rec_n);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
