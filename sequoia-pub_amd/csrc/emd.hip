// Earth mover's distance of two maps on the device (include/sequoia_hip.h, "Earth mover's distance"): the grid fill and shift
// of spatial_vis/get_emd.py:180-188, calculate_emd's conventions (:67-90) and, where the reference calls cv2.EMD, the optimum
// of the balanced transportation problem in f64 with its certificate (flow + duals).
//   fill        one workgroup per problem: the extents over the present rows, both grids zeroed, every row's number scattered
//               into an int32 owner grid (two rows of one cell: one wins, the other finds out and raises the flag), the values
//               written, the minimum over the WHOLE grid taken and arr + abs(min) applied -- the literal steps.
//   signature   one workgroup per (problem, map): the f64 sum in a fixed order, then the cells with weight > 0 compacted in
//               row-major order (wave ballots, the waves' counts through LDS), weight = value / sum.
//   solve       one workgroup per problem, successive shortest augmenting paths.  Sources (map a) are rows, sinks (map b) are
//               columns.  The columns' labels d, duals v, predecessors, coordinates, arc-list heads and flags and the rows'
//               duals u, coordinates and scanned bits sit in LDS (38.1 bytes a cell: 153 KiB at the cell limit); the arc pool
//               and what only an augmentation reads are in global memory and only thread 0 walks them.  A search step:
//               every thread relaxes its columns (tid, tid + EMD_THREADS, ...) from the rows scanned since the last step
//               (thread 0 stages them in LDS as it finds them, EMD_STAGE at a time), the workgroup takes the argmin over
//               the unfinalised columns (lowest index on ties), thread 0 finalises it and follows its flow arcs back to
//               unscanned rows: two barriers and one dependent global load (the arc) per step.  The first finalised
//               column with demand left ends the search at distance D: v_j -= D - d_j on the finalised columns, u_i +=
//               D - dist_i on the scanned rows, and thread 0 augments along the predecessors.  Arcs whose flow returns to 0
//               go back to the pool's free list.  Work is bounded by max_aug augmentations and arc_cap arc slots; reaching
//               either ends the problem with its status.  No workgroup reads what another writes.
// Everything is a separately rounded f64 operation in a fixed order; the only atomics are integer ones in LDS.  Two calls
// give the same bytes.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EMD_THREADS = 256;          // the column chunk: columns one pass of the workgroup covers
constexpr int EMD_WAVES = EMD_THREADS / 64;
constexpr int EMD_STAGE = 64;             // newly scanned rows staged in LDS per relax pass
constexpr int EMD_SIG_BAD = 1, EMD_SIG_MANY = 2;

__device__ __forceinline__ int emd_pack(int cell, int W) { return ((cell / W) << 16) | (cell % W); }
__device__ __forceinline__ double emd_cost(int a, int b) {
    const int dx = (a >> 16) - (b >> 16), dy = (a & 0xFFFF) - (b & 0xFFFF);
    return __dsqrt_rn((double)(dx * dx + dy * dy));
}

// the sum of one value per thread in a fixed tree; every thread gets it
__device__ __forceinline__ double emd_block_sum(double x, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int s = EMD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ------------------------------------------------------------------------------------------
// 1. grid fill and shift (get_emd.py:180-188)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EMD_THREADS) void emd_fill_kernel(const double* __restrict__ a, int lda, const int32_t* __restrict__ cols_a,
                                                               const double* __restrict__ b, int ldb, const int32_t* __restrict__ cols_b, int n,
                                                               const int32_t* __restrict__ xtf, const int32_t* __restrict__ ytf, int nan_absent,
                                                               int gh, int gw, int cells, double* grids, int32_t* __restrict__ dims,
                                                               uint8_t* __restrict__ flag, int32_t* owner_all) {
    __shared__ int s_mx, s_my, s_nan[2];
    __shared__ double red[2][EMD_THREADS];
    const int tid = threadIdx.x, p = blockIdx.x;
    const size_t ca = (size_t)(cols_a ? cols_a[p] : p), cb = (size_t)(cols_b ? cols_b[p] : p);
    double* const ga = grids + (size_t)p * 2 * (size_t)cells;
    double* const gb = ga + cells;
    int32_t* const own = owner_all + (size_t)p * (size_t)cells;
    if (tid == 0) { s_mx = -1; s_my = -1; s_nan[0] = 0; s_nan[1] = 0; }
    __syncthreads();
    int mx = -1, my = -1;
    for (int i = tid; i < n; i += EMD_THREADS) {
        const double va = a[(size_t)i * (size_t)lda + ca], vb = b[(size_t)i * (size_t)ldb + cb];
        if (nan_absent && (va != va || vb != vb)) continue;
        const int x = xtf[i], y = ytf[i];
        if (x < 0 || x >= gh || y < 0 || y >= gw) { flag[0] = 1; continue; }        // every writer stores the same value
        mx = max(mx, x);
        my = max(my, y);
    }
    atomicMax(&s_mx, mx);                                     // integer maxima in LDS: the order does not matter
    atomicMax(&s_my, my);
    __syncthreads();
    const int H = s_mx + 1, W = s_my + 1, N = H * W;          // N <= gh gw <= cells
    if (tid == 0) { dims[2 * p] = H; dims[2 * p + 1] = W; }
    for (int c = tid; c < N; c += EMD_THREADS) { ga[c] = 0.0; gb[c] = 0.0; own[c] = -1; }
    __syncthreads();
    for (int i = tid; i < n; i += EMD_THREADS) {
        const double va = a[(size_t)i * (size_t)lda + ca], vb = b[(size_t)i * (size_t)ldb + cb];
        if (nan_absent && (va != va || vb != vb)) continue;
        const int x = xtf[i], y = ytf[i];
        if (x < 0 || x >= gh || y < 0 || y >= gw) continue;
        own[x * W + y] = i;
    }
    __syncthreads();
    for (int i = tid; i < n; i += EMD_THREADS) {
        const double va = a[(size_t)i * (size_t)lda + ca], vb = b[(size_t)i * (size_t)ldb + cb];
        if (nan_absent && (va != va || vb != vb)) continue;
        const int x = xtf[i], y = ytf[i];
        if (x < 0 || x >= gh || y < 0 || y >= gw) continue;
        const int c = x * W + y;
        if (own[c] != i) { flag[0] = 1; continue; }
        ga[c] = va;
        gb[c] = vb;
    }
    __syncthreads();
    double ma = INFINITY, mb = INFINITY;
    for (int c = tid; c < N; c += EMD_THREADS) {
        const double x = ga[c], y = gb[c];
        if (x != x) s_nan[0] = 1;                             // np.min of a grid holding a NaN is NaN
        if (y != y) s_nan[1] = 1;
        ma = x < ma ? x : ma;
        mb = y < mb ? y : mb;
    }
    red[0][tid] = ma;
    red[1][tid] = mb;
    __syncthreads();
    for (int s = EMD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = red[0][tid + s] < red[0][tid] ? red[0][tid + s] : red[0][tid];
            red[1][tid] = red[1][tid + s] < red[1][tid] ? red[1][tid + s] : red[1][tid];
        }
        __syncthreads();
    }
    const double sa = s_nan[0] ? __builtin_nan("") : fabs(red[0][0]), sb = s_nan[1] ? __builtin_nan("") : fabs(red[1][0]);
    for (int c = tid; c < N; c += EMD_THREADS) {
        ga[c] = ga[c] + sa;
        gb[c] = gb[c] + sb;
    }
}

// ------------------------------------------------------------------------------------------
// 2. signatures: normalise, keep the cells with weight > 0 (calculate_emd :71-82, cv2's skipped zero weights)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EMD_THREADS) void emd_signature_kernel(const double* __restrict__ grids, int cells, const int32_t* __restrict__ dims,
                                                                    int cap, double* __restrict__ sums, int32_t* __restrict__ sig,
                                                                    int32_t* __restrict__ cell_a, double* __restrict__ w_a,
                                                                    int32_t* __restrict__ cell_b, double* __restrict__ w_b) {
    __shared__ double red[EMD_THREADS];
    __shared__ int s_bad, wtot[EMD_WAVES];
    const int tid = threadIdx.x, side = blockIdx.x, p = blockIdx.y, lane = tid & 63, wave = tid >> 6;
    const int H = dims[2 * p], W = dims[2 * p + 1];
    const bool bad_dims = H < 0 || W < 0 || H > SQ_EMD_MAX_DIM || W > SQ_EMD_MAX_DIM || (long long)H * (long long)W > (long long)cells;
    const int N = bad_dims ? 0 : H * W;
    const double* const g = grids + ((size_t)p * 2 + (size_t)side) * (size_t)cells;
    int32_t* const cell_out = (side ? cell_b : cell_a) + (size_t)p * (size_t)cap;
    double* const w_out = (side ? w_b : w_a) + (size_t)p * (size_t)cap;
    if (tid == 0) s_bad = bad_dims ? 1 : 0;
    double s = 0.0;
    bool neg = false;
    for (int c = tid; c < N; c += EMD_THREADS) {
        const double x = g[c];
        s = s + x;
        neg = neg || !(x >= 0.0);
    }
    const double total = emd_block_sum(s, red);
    if (neg || !(total < INFINITY)) s_bad = 1;
    __syncthreads();
    int base = 0;
    if (!s_bad && total > 0.0) {
        for (int c0 = 0; c0 < N; c0 += EMD_THREADS) {
            const int c = c0 + tid;
            const double w = c < N ? g[c] / total : 0.0;
            const bool keep = w > 0.0;
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wtot[wave] = __popcll(m);
            __syncthreads();
            int off = base + __popcll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
            for (int q = 0; q < EMD_WAVES; ++q) {
                if (q < wave) off += wtot[q];
                all += wtot[q];
            }
            if (keep && off < cap) { cell_out[off] = c; w_out[off] = w; }
            base += all;
            __syncthreads();
        }
    }
    if (tid == 0) {
        const int q = p * 2 + side;
        sums[q] = total;
        sig[3 * q] = s_bad ? EMD_SIG_BAD : (base > cap ? EMD_SIG_MANY : 0);
        sig[3 * q + 1] = base;
        sig[3 * q + 2] = bad_dims ? 1 : W;
    }
}

// ------------------------------------------------------------------------------------------
// 3. the transportation problem
// ------------------------------------------------------------------------------------------
struct EmdWs {                // per-problem global state, offsets in bytes from the problem's base
    size_t dist, pred_col, pred_arc, scanlist, brem, next, per_problem;
};

EmdWs emd_ws(int cap, int arc_cap) {
    EmdWs w;
    size_t o = 0;
    w.dist = o;     o += sq_align_up((size_t)cap * 8, 256);
    w.brem = o;     o += sq_align_up((size_t)cap * 8, 256);
    w.pred_col = o; o += sq_align_up((size_t)cap * 4, 256);
    w.pred_arc = o; o += sq_align_up((size_t)cap * 4, 256);
    w.scanlist = o; o += sq_align_up((size_t)cap * 4, 256);
    w.next = o;     o += sq_align_up((size_t)arc_cap * 4, 256);
    w.per_problem = o;
    return w;
}

// d, v, u (f64), cxy, rxy (int32), the scanned rows' bit mask, pred, head (uint16), fin, dem (bytes) for cap columns and cap rows
__host__ __device__ constexpr int emd_scan_words(int cap) { return (cap + 31) / 32; }
size_t emd_lds_bytes(int cap) { return (size_t)cap * (3 * 8 + 2 * 4 + 2 * 2 + 2) + (size_t)emd_scan_words(cap) * 4; }

constexpr unsigned short EMD_NONE = 0xFFFF;                   // no predecessor row / no arc: rows < 4096 and arc slots < 16384 are below it

__global__ __launch_bounds__(EMD_THREADS) void emd_solve_kernel(int cap, int arc_cap, int max_aug_arg, const double* __restrict__ sums,
                                                                const int32_t* __restrict__ sig, EmdWs lay, char* ws_all, double* __restrict__ value,
                                                                int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ cell_a_all, const double* __restrict__ w_a_all,
                                                                const int32_t* __restrict__ cell_b_all, const double* __restrict__ w_b_all,
                                                                double* __restrict__ u_all, double* __restrict__ v_all, int32_t* arc_i_all,
                                                                int32_t* arc_j_all, double* arc_f_all) {
    extern __shared__ double emd_smem[];
    double* const d = emd_smem;                               // label of a column in the running search
    double* const v = d + cap;                                // dual of a column
    double* const u = v + cap;                                // dual of a row
    int* const cxy = (int*)(u + cap);                         // packed coordinates of a column's cell
    int* const rxy = cxy + cap;                               // ... of a row's cell
    unsigned* const scan = (unsigned*)(rxy + cap);            // bit r: row r is scanned in the running search
    unsigned short* const pred = (unsigned short*)(scan + emd_scan_words(cap));      // the row a column's label came from
    unsigned short* const head = pred + cap;                  // first arc of a column's flow list
    unsigned char* const fin = (unsigned char*)(head + cap);  // finalised in the running search
    unsigned char* const dem = fin + cap;                     // demand left
    __shared__ double red[EMD_THREADS];
    __shared__ double red_val[EMD_WAVES], st_base[EMD_STAGE], s_D, s_supply;
    __shared__ int red_idx[EMD_WAVES], st_xy[EMD_STAGE], st_row[EMD_STAGE];
    __shared__ int s_stop, s_jstar, s_prev, s_nscan, s_ndem, s_status, s_naug, s_free, s_bump, s_steps;

    const int tid = threadIdx.x, p = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sa = sig[6 * p], na = sig[6 * p + 1], wa_ = sig[6 * p + 2], sb = sig[6 * p + 3], nb = sig[6 * p + 4], wb_ = sig[6 * p + 5];
    const double sum_a = sums[2 * p], sum_b = sums[2 * p + 1];
    int32_t* const cnt = counts + 8 * (size_t)p;
    if (sa || sb || sum_a == 0.0 || sum_b == 0.0) {           // uniform over the workgroup: everyone leaves
        if (tid == 0) {
            const bool bad = sa == EMD_SIG_BAD || sb == EMD_SIG_BAD, many = sa == EMD_SIG_MANY || sb == EMD_SIG_MANY;
            status[p] = bad ? SQ_EMD_BAD_GRID : many ? SQ_EMD_TOO_MANY_CELLS : SQ_EMD_OK;
            value[p] = (!bad && !many && sum_a == 0.0 && sum_b == 0.0) ? 0.0 : __builtin_nan("");      // :71-79
            cnt[0] = na; cnt[1] = nb; cnt[2] = 0; cnt[3] = 0; cnt[4] = 0; cnt[5] = 0; cnt[6] = 0; cnt[7] = 0;
        }
        return;
    }
    char* const ws = ws_all + (size_t)p * lay.per_problem;
    double* const dist = (double*)(ws + lay.dist);            // a scanned row's distance in the running search
    double* const brem = (double*)(ws + lay.brem);            // a column's remaining demand
    int* const pred_col = (int*)(ws + lay.pred_col);          // the column a row was reached from, and through which arc
    int* const pred_arc = (int*)(ws + lay.pred_arc);
    int* const scanlist = (int*)(ws + lay.scanlist);          // the scanned rows in the order they were reached
    int* const nxt = (int*)(ws + lay.next);                   // next arc of a column's list, or of the free list; -1: none
    const int32_t* const cell_a = cell_a_all + (size_t)p * (size_t)cap;
    const int32_t* const cell_b = cell_b_all + (size_t)p * (size_t)cap;
    const double* const w_a = w_a_all + (size_t)p * (size_t)cap;
    const double* const w_b = w_b_all + (size_t)p * (size_t)cap;
    int32_t* const arc_i = arc_i_all + (size_t)p * (size_t)arc_cap;
    int32_t* const arc_j = arc_j_all + (size_t)p * (size_t)arc_cap;
    double* const arc_f = arc_f_all + (size_t)p * (size_t)arc_cap;
    const int max_aug = max_aug_arg > 0 ? max_aug_arg : SQ_EMD_DEFAULT_AUGMENTATIONS * (na + nb);

    for (int j = tid; j < nb; j += EMD_THREADS) {
        cxy[j] = emd_pack(cell_b[j], wb_);
        brem[j] = w_b[j];
        dem[j] = 1; fin[j] = 0; d[j] = INFINITY; head[j] = EMD_NONE; pred[j] = EMD_NONE;
    }
    for (int i = tid; i < na; i += EMD_THREADS) { rxy[i] = emd_pack(cell_a[i], wa_); u[i] = 0.0; }
    for (int w = tid; w < emd_scan_words(cap); w += EMD_THREADS) scan[w] = 0u;
    for (int s = tid; s < arc_cap; s += EMD_THREADS) { arc_f[s] = 0.0; arc_i[s] = -1; arc_j[s] = -1; }
    if (tid == 0) { s_ndem = nb; s_status = 0; s_naug = 0; s_free = -1; s_bump = 0; s_steps = 0; s_supply = 0.0; }
    __syncthreads();
    for (int j = tid; j < nb; j += EMD_THREADS) {             // v_j = min_i c_ij: the square root is monotone
        const int b = cxy[j];
        int best = 0x7FFFFFFF;
        for (int i = 0; i < na; ++i) {
            const int a = rxy[i];
            const int dx = (a >> 16) - (b >> 16), dy = (a & 0xFFFF) - (b & 0xFFFF);
            best = min(best, dx * dx + dy * dy);
        }
        v[j] = __dsqrt_rn((double)best);
    }

    for (int s = 0; s < na; ++s) {
        __syncthreads();
        if (s_status != 0 || s_ndem == 0) break;
        __syncthreads();
        if (tid == 0) s_supply = w_a[s];
        for (;;) {
            __syncthreads();                                  // thread 0's state of the previous round is visible
            const double supply = s_supply;
            const int ndem = s_ndem, stt = s_status, naug = s_naug;
            __syncthreads();                                  // and read by everyone before thread 0 changes it
            if (!(supply > 0.0) || ndem == 0 || stt != 0) break;
            if (naug >= max_aug) {
                if (tid == 0) s_status = SQ_EMD_AUGMENTATION_CAP;
                break;
            }
            if (tid == 0) {                                   // the search starts at row s, staged for the first relax pass
                scan[s >> 5] |= 1u << (s & 31);
                dist[s] = 0.0; scanlist[0] = s;
                st_row[0] = s; st_xy[0] = rxy[s]; st_base[0] = 0.0 - u[s];
                s_prev = 0; s_nscan = 1; s_stop = 0;
            }
            __syncthreads();
            for (;;) {                                        // one search step per round
                const int prev = s_prev, nscan = s_nscan;
                for (int c0 = prev; c0 < nscan; c0 += EMD_STAGE) {
                    const int len = min(EMD_STAGE, nscan - c0);
                    if (c0 > prev) {                          // thread 0 staged the first EMD_STAGE new rows; the rest comes from the list
                        __syncthreads();
                        if (tid < len) {
                            const int r = scanlist[c0 + tid];
                            st_row[tid] = r;
                            st_xy[tid] = rxy[r];
                            st_base[tid] = dist[r] - u[r];
                        }
                        __syncthreads();
                    }
                    for (int j = tid; j < nb; j += EMD_THREADS) {
                        if (fin[j]) continue;
                        const int b = cxy[j];
                        const double vj = v[j];
                        double dj = d[j];
                        int pj = pred[j];
                        for (int k = 0; k < len; ++k) {
                            const double val = (emd_cost(st_xy[k], b) - vj) + st_base[k];
                            if (val < dj) { dj = val; pj = st_row[k]; }
                        }
                        d[j] = dj;
                        pred[j] = (unsigned short)pj;
                    }
                }
                double best = INFINITY;
                int bj = 0x7FFFFFFF;
                for (int j = tid; j < nb; j += EMD_THREADS)
                    if (!fin[j] && d[j] < best) { best = d[j]; bj = j; }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ov = __shfl_down(best, o, 64);
                    const int oi = __shfl_down(bj, o, 64);
                    if (ov < best || (ov == best && oi < bj)) { best = ov; bj = oi; }
                }
                if (lane == 0) { red_val[wave] = best; red_idx[wave] = bj; }
                __syncthreads();                              // every relax pass has read the staged rows
                if (tid == 0) {
                    best = red_val[0]; bj = red_idx[0];
#pragma unroll
                    for (int q = 1; q < EMD_WAVES; ++q)
                        if (red_val[q] < best || (red_val[q] == best && red_idx[q] < bj)) { best = red_val[q]; bj = red_idx[q]; }
                    ++s_steps;
                    if (bj == 0x7FFFFFFF) {
                        s_stop = 2;
                    } else {
                        fin[bj] = 1;
                        s_D = best;
                        s_jstar = bj;
                        if (dem[bj]) {
                            s_stop = 1;
                        } else {
                            int ns = nscan;
                            for (int a = head[bj] == EMD_NONE ? -1 : (int)head[bj]; a >= 0; a = nxt[a]) {
                                const int r = arc_i[a];
                                if (scan[r >> 5] >> (r & 31) & 1u) continue;
                                scan[r >> 5] |= 1u << (r & 31);
                                dist[r] = best; pred_col[r] = bj; pred_arc[r] = a; scanlist[ns] = r;
                                if (ns - nscan < EMD_STAGE) {
                                    const int k = ns - nscan;
                                    st_row[k] = r; st_xy[k] = rxy[r]; st_base[k] = best - u[r];
                                }
                                ++ns;
                            }
                            s_prev = nscan;
                            s_nscan = ns;
                        }
                    }
                }
                __syncthreads();
                if (s_stop) break;
            }
            if (s_stop == 2) {
                if (tid == 0) s_status = SQ_EMD_NO_PATH;
                continue;                                     // the round's first barrier, then everyone leaves
            }
            const double D = s_D;
            const int nscan = s_nscan;
            for (int j = tid; j < nb; j += EMD_THREADS) {
                if (fin[j]) { v[j] = v[j] - (D - d[j]); fin[j] = 0; }
                d[j] = INFINITY;
            }
            for (int k = tid; k < nscan; k += EMD_THREADS) {
                const int r = scanlist[k];
                u[r] = u[r] + (D - dist[r]);
            }
            for (int w = tid; w < emd_scan_words(cap); w += EMD_THREADS) scan[w] = 0u;
            __syncthreads();
            if (tid == 0) {                                   // augment along the predecessors
                const int jst = s_jstar;
                double delta = s_supply < brem[jst] ? s_supply : brem[jst];
                bool whole = true;                            // the predecessors lead back to s within na rows: a tree
                for (int j = jst, steps = 0;; ++steps) {
                    const int r = pred[j];
                    if (r == s) break;
                    if (r >= na || steps >= na) { whole = false; break; }
                    const double f = arc_f[pred_arc[r]];
                    delta = f < delta ? f : delta;
                    j = pred_col[r];
                }
                if (!whole) s_status = SQ_EMD_NO_PATH;
                for (int j = jst; whole;) {
                    const int r = pred[j];
                    int a = head[j] == EMD_NONE ? -1 : (int)head[j];
                    while (a >= 0 && arc_i[a] != r) a = nxt[a];
                    if (a >= 0) {
                        arc_f[a] = arc_f[a] + delta;
                    } else {
                        if (s_free >= 0) { a = s_free; s_free = nxt[a]; }
                        else if (s_bump < arc_cap) a = s_bump++;
                        else { s_status = SQ_EMD_ARC_CAP; break; }
                        arc_i[a] = r; arc_j[a] = j; arc_f[a] = delta;
                        nxt[a] = head[j] == EMD_NONE ? -1 : (int)head[j];
                        head[j] = (unsigned short)a;
                    }
                    if (r == s) break;
                    const int ab = pred_arc[r], jb = pred_col[r];
                    const double f = arc_f[ab] - delta;
                    if (f > 0.0) {
                        arc_f[ab] = f;
                    } else {                                  // the arc leaves the flow: unlink it, its slot is free again
                        if ((int)head[jb] == ab) {
                            head[jb] = nxt[ab] < 0 ? EMD_NONE : (unsigned short)nxt[ab];
                        } else {
                            int q = head[jb] == EMD_NONE ? -1 : (int)head[jb];
                            while (q >= 0 && nxt[q] != ab) q = nxt[q];
                            if (q >= 0) nxt[q] = nxt[ab];
                        }
                        arc_f[ab] = 0.0; arc_i[ab] = -1; arc_j[ab] = -1;
                        nxt[ab] = s_free; s_free = ab;
                    }
                    j = jb;
                }
                s_supply = s_supply - delta;
                const double left = brem[jst] - delta;
                brem[jst] = left;
                if (!(left > 0.0)) { dem[jst] = 0; --s_ndem; }
                ++s_naug;
            }
        }
    }
    __syncthreads();
    double* const vo = v_all + (size_t)p * (size_t)cap;
    double* const uo = u_all + (size_t)p * (size_t)cap;
    for (int j = tid; j < nb; j += EMD_THREADS) vo[j] = v[j];
    for (int i = tid; i < na; i += EMD_THREADS) uo[i] = u[i];
    double part = 0.0;
    for (int s = tid; s < arc_cap; s += EMD_THREADS) {
        const double f = arc_f[s];
        if (f > 0.0) part = part + f * emd_cost(rxy[arc_i[s]], cxy[arc_j[s]]);
    }
    const double total = emd_block_sum(part, red);
    if (tid == 0) {
        status[p] = s_status;
        value[p] = s_status ? __builtin_nan("") : total;
        cnt[0] = na; cnt[1] = nb; cnt[2] = s_naug; cnt[3] = s_bump; cnt[4] = s_steps; cnt[5] = 0; cnt[6] = 0; cnt[7] = 0;
    }
}

SqDevOnce emd_attr_once;

}  // namespace

static_assert(EMD_THREADS == 256 && EMD_STAGE <= EMD_THREADS, "the reductions are written for four waves");
static_assert(SQ_EMD_MAX_CELLS * 38 + SQ_EMD_MAX_CELLS / 8 + 4096 <= 160 * 1024, "the columns' and rows' state at the cell limit fits the CU's 160 KiB of LDS");
static_assert(SQ_EMD_MAX_CELLS < 0xFFFF && SQ_EMD_MAX_ARCS < 0xFFFF, "rows and arc slots fit 16 bits below EMD_NONE");
static_assert(SQ_EMD_MAX_DIM <= 32768, "a cell's coordinates pack into 2 x 16 bits and dx dx + dy dy fits an int");

extern "C" int sq_emd_column_chunk(void) { return EMD_THREADS; }

extern "C" const char* sq_emd_status_text(int status) {
    switch (status) {
        case SQ_EMD_OK: return "solved";
        case SQ_EMD_TOO_MANY_CELLS: return "a map has more cells of positive weight than cap_cells";
        case SQ_EMD_AUGMENTATION_CAP: return "the cap on augmentations was reached with supply left";
        case SQ_EMD_ARC_CAP: return "the flow needs more arcs than arc_cap";
        case SQ_EMD_BAD_GRID: return "a grid extent is out of range or a grid holds a negative or non-finite value";
        case SQ_EMD_NO_PATH: return "a search ended without reaching demand";
        default: return "unknown status";
    }
}

extern "C" int sq_emd_status_check(const int32_t* status_host, int P) {
    SQ_REQUIRE(status_host && P >= 1, "emd_status_check: null status or P = %d", P);
    for (int p = 0; p < P; ++p)
        if (status_host[p] != SQ_EMD_OK) {
            sq_set_error("emd_solve: problem %d ended with status %d: %s", p, status_host[p], sq_emd_status_text(status_host[p]));
            return SQ_ERR_UNSUPPORTED;
        }
    return SQ_OK;
}

extern "C" size_t sq_emd_fill_workspace_bytes(int P, int cells) {
    if (P < 1 || P > SQ_EMD_MAX_PROBLEMS || cells < 1 || cells > SQ_EMD_MAX_GRID_CELLS) return 0;
    return sq_align_up((size_t)P * (size_t)cells * 4, 256);
}

extern "C" int sq_emd_fill(const double* a, int lda, const int32_t* cols_a, const double* b, int ldb, const int32_t* cols_b, int n,
                           const int32_t* xtf, const int32_t* ytf, int P, int nan_absent, int grid_h, int grid_w, int cells, double* grids,
                           int32_t* dims, uint8_t* flag, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE_ROWS("emd_fill", n, 1, SQ_MAP_MAX_ROWS);
    SQ_REQUIRE(P >= 1 && P <= SQ_EMD_MAX_PROBLEMS, "emd_fill: P = %d problems, must be in 1..%d", P, SQ_EMD_MAX_PROBLEMS);
    SQ_REQUIRE(lda >= 1 && ldb >= 1 && (cols_a || P <= lda) && (cols_b || P <= ldb),
               "emd_fill: leading dimensions lda = %d, ldb = %d for P = %d problems (no column list: P <= ld)", lda, ldb, P);
    SQ_REQUIRE(grid_h >= 1 && grid_w >= 1 && grid_h <= SQ_EMD_MAX_DIM && grid_w <= SQ_EMD_MAX_DIM, "emd_fill: grid %d x %d, both extents must be in 1..%d",
               grid_h, grid_w, SQ_EMD_MAX_DIM);
    SQ_REQUIRE(cells >= 1 && cells <= SQ_EMD_MAX_GRID_CELLS && (long long)grid_h * (long long)grid_w <= (long long)cells,
               "emd_fill: cells = %d, must hold the grid %d x %d and be at most %d", cells, grid_h, grid_w, SQ_EMD_MAX_GRID_CELLS);
    SQ_REQUIRE(nan_absent == 0 || nan_absent == 1, "emd_fill: nan_absent = %d, must be 0 or 1", nan_absent);
    SQ_REQUIRE(a && b && xtf && ytf && grids && dims && flag && workspace, "emd_fill: null a, b, xtf, ytf, grids, dims, flag or workspace pointer");
    SQ_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)grids | (uintptr_t)workspace) & 7) == 0 &&
               (((uintptr_t)cols_a | (uintptr_t)cols_b | (uintptr_t)xtf | (uintptr_t)ytf | (uintptr_t)dims) & 3) == 0, "emd_fill: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("emd_fill", workspace_bytes, sq_emd_fill_workspace_bytes(P, cells));
    hipLaunchKernelGGL(emd_fill_kernel, dim3((unsigned)P), dim3(EMD_THREADS), 0, (hipStream_t)stream_, a, lda, cols_a, b, ldb, cols_b, n, xtf, ytf,
                       nan_absent, grid_h, grid_w, cells, grids, dims, flag, (int32_t*)workspace);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

extern "C" size_t sq_emd_workspace_bytes(int P, int cap_cells, int arc_cap) {
    if (P < 1 || P > SQ_EMD_MAX_PROBLEMS || cap_cells < 1 || cap_cells > SQ_EMD_MAX_CELLS || arc_cap < 1 || arc_cap > SQ_EMD_MAX_ARCS) return 0;
    return sq_align_up((size_t)P * 2 * 8, 256) + sq_align_up((size_t)P * 6 * 4, 256) + (size_t)P * emd_ws(cap_cells, arc_cap).per_problem;
}

extern "C" int sq_emd_solve(const double* grids, int cells, const int32_t* dims, int P, int cap_cells, int arc_cap, int max_aug, double* value,
                            int32_t* status, int32_t* counts, int32_t* cell_a, double* w_a, int32_t* cell_b, double* w_b, double* u, double* v,
                            int32_t* arc_i, int32_t* arc_j, double* arc_f, void* workspace, size_t workspace_bytes, sq_stream_t stream_) {
    SQ_REQUIRE(P >= 1 && P <= SQ_EMD_MAX_PROBLEMS, "emd_solve: P = %d problems, must be in 1..%d", P, SQ_EMD_MAX_PROBLEMS);
    SQ_REQUIRE(cells >= 1 && cells <= SQ_EMD_MAX_GRID_CELLS, "emd_solve: cells = %d, must be in 1..%d", cells, SQ_EMD_MAX_GRID_CELLS);
    SQ_REQUIRE(cap_cells >= 1 && cap_cells <= SQ_EMD_MAX_CELLS, "emd_solve: cap_cells = %d, must be in 1..%d", cap_cells, SQ_EMD_MAX_CELLS);
    SQ_REQUIRE(arc_cap >= 1 && arc_cap <= SQ_EMD_MAX_ARCS, "emd_solve: arc_cap = %d, must be in 1..%d", arc_cap, SQ_EMD_MAX_ARCS);
    SQ_REQUIRE(max_aug >= 0, "emd_solve: max_aug = %d, must be at least 0 (0: %d (na + nb))", max_aug, SQ_EMD_DEFAULT_AUGMENTATIONS);
    SQ_REQUIRE(grids && dims && value && status && counts && cell_a && w_a && cell_b && w_b && u && v && arc_i && arc_j && arc_f && workspace,
               "emd_solve: null grids, dims, output or workspace pointer");
    SQ_REQUIRE((((uintptr_t)grids | (uintptr_t)value | (uintptr_t)w_a | (uintptr_t)w_b | (uintptr_t)u | (uintptr_t)v | (uintptr_t)arc_f |
                 (uintptr_t)workspace) & 7) == 0 &&
               (((uintptr_t)dims | (uintptr_t)status | (uintptr_t)counts | (uintptr_t)cell_a | (uintptr_t)cell_b | (uintptr_t)arc_i | (uintptr_t)arc_j) & 3) == 0,
               "emd_solve: misaligned pointer");
    SQ_REQUIRE_WORKSPACE("emd_solve", workspace_bytes, sq_emd_workspace_bytes(P, cap_cells, arc_cap));
    hipStream_t st = (hipStream_t)stream_;
    char* const ws = (char*)workspace;
    double* const sums = (double*)ws;
    int32_t* const sig = (int32_t*)(ws + sq_align_up((size_t)P * 2 * 8, 256));
    char* const per = ws + sq_align_up((size_t)P * 2 * 8, 256) + sq_align_up((size_t)P * 6 * 4, 256);
    const EmdWs lay = emd_ws(cap_cells, arc_cap);
    if (emd_attr_once.needed()) {
        SQ_HIP_CHECK(hipFuncSetAttribute((const void*)emd_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)emd_lds_bytes(SQ_EMD_MAX_CELLS)));
        emd_attr_once.done();
    }
    hipLaunchKernelGGL(emd_signature_kernel, dim3(2, (unsigned)P), dim3(EMD_THREADS), 0, st, grids, cells, dims, cap_cells, sums, sig, cell_a, w_a,
                       cell_b, w_b);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(emd_solve_kernel, dim3((unsigned)P), dim3(EMD_THREADS), emd_lds_bytes(cap_cells), st, cap_cells, arc_cap, max_aug,
                       (const double*)sums, (const int32_t*)sig, lay, per, value, status, counts, (const int32_t*)cell_a, (const double*)w_a,
                       (const int32_t*)cell_b, (const double*)w_b, u, v, arc_i, arc_j, arc_f);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}
