// Per-slide k-Means(100) + cluster means on the GPU, batched over slides.
//
// Stands behind pre_processing/kmean_features.py:96-108:
//     KMeans(n_clusters=100, random_state=0).fit(features).labels_ ; per-label np.mean
// i.e. scikit-learn's KMeans defaults (k-means++ seeding with 2+log(k) local trials, Lloyd,
// max_iter 300, tol 1e-4) with the arithmetic defined in oracle/kmeans_oracle.py:
//   * centring: column mean by adding rows in index order in fp32, X - mean in fp32
//   * seeding distances  fl32(max(0, (-2 x.c + |x|^2) + |c|^2)) with fp64 dot products -- every
//     candidate is a data point, so all of them come from ONE fp64 Gram matrix G = Xc Xc^T
//     (v_mfma_f64_16x16x4_f64); the 99 dependent seeding steps then only read rows of G
//   * potentials fl32(sum_fp64), cumsum in fp64, searchsorted(side=left), first-minimum argmin
//   * Lloyd: |c|^2 - 2 x.c in fp64 on fp32 centres (fp64 MFMA), strict-< argmin, fp64 member
//     sums in index order, fl32(sum/count), empty-cluster relocation, centre-shift / label stop rule
//   * cluster means of the ORIGINAL features: member rows added in index order in fp32, / count
// One workgroup per slide runs the whole seeding loop; slides are independent (grid dimension).
// A call's slides lie back to back and are described by ONE slide table in device memory (KmSlide), which every kernel
// that touches per-point data reads.  One driver (km_fit, section 6) stands behind the three entries, which differ in
// how the table is filled: sq_kmeans_fit S equal slides, sq_kmeans_fit_ragged slides of different row counts (each
// <= 4096), sq_kmeans_fit_large one slide of up to 65536 points (compute_features_hdf5.py:26,112-113:
// --max_patch_number is the user's).  The large route keeps the arithmetic without the n x n Gram matrix -- a seeding
// step forms only its candidates' distances, `closest` lives in global memory, member lists come from a chunked
// counting sort (section 5); centring, the centre gather and the Lloyd loop are the same launches for all three.
#include "../../include/sequoia_hip.h"
#include "sq_common.h"

#include <vector>

namespace {

constexpr int KM_THREADS = 1024;
constexpr int KM_MAX_TRIALS = 8;
constexpr int KM_MAX_K = 256;
constexpr int KM_DOT_SLICES = 8;        // K slices of the centre x point products

struct KmState {          // per slide, device memory
    int iter;             // Lloyd iterations run
    int done;             // 1 once converged / max_iter reached
    int strict;           // labels unchanged between two iterations
    int n_empty;          // empty clusters found in the current iteration
    double tol;           // 1e-4 * mean(var(X, axis=0))
    double shift;         // sum of squared centre shifts of the current iteration
};

// Where slide s keeps its rows and its n x n tables: one entry of the call's slide table (device memory), which every
// kernel that touches per-point data reads.  The slides lie back to back: buffers linear in n (Xc, labels, labels_old,
// members, dist, the dots planes) start at `row` times their row width, G and dist32 at `gram`; buffers sized per slide
// ([S][k]...) are indexed by s alone.
struct KmSlide {
    int n;                // rows of the slide
    int first;            // its first centre
    size_t row;           // rows of the slides before it
    size_t gram;          // elements of their n x n tables (each rounded up to 4: 16-byte rows for the seeding loads)
};
static inline size_t km_gram_elems(int n) { return sq_align_up((size_t)n * n, 4); }

// The table of S equal slides and, behind it, the identity list (every slide is of one seeding class), filled where
// they are read: a lone slide's call is too short to pay for a host block and its copy.
__global__ void km_equal_table_kernel(KmSlide* __restrict__ tab, int* __restrict__ list, int S, int n, int first, size_t gram) {
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        tab[s] = KmSlide{n, first, (size_t)s * n, (size_t)s * gram};
        list[s] = s;
    }
}

// ------------------------------------------------------------------------------------------
// block-wide helpers (blockDim.x multiple of 64, <= 1024)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_reduce_sum(double v, double* sh /*[16]*/) {
    v = wave_sum_f64(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < nw; ++i) r += sh[i];     // same order on every thread -> identical result
    return r;
}

__device__ __forceinline__ int block_reduce_sum_int(int v, int* sh /*[16]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wv] = v;
    __syncthreads();
    int r = 0;
    for (int i = 0; i < nw; ++i) r += sh[i];
    return r;
}

// T values per thread reduced together: 2 barriers for the whole set (the seeding loop is barrier-latency bound)
template <int T>
__device__ __forceinline__ void block_reduce_sum_n(double (&v)[T], double* sh /*[16 * T]*/) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = wave_sum_f64(v[t]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) sh[wv * T + t] = v[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double r = 0.0;
        for (int i = 0; i < nw; ++i) r += sh[i * T + t];
        v[t] = r;
    }
}

template <int T>
__device__ __forceinline__ void block_reduce_sum_n_int(int (&v)[T], int* sh /*[16 * T]*/) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[t] += __shfl_xor(v[t], o, 64);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) sh[wv * T + t] = v[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t) {
        int r = 0;
        for (int i = 0; i < nw; ++i) r += sh[i * T + t];
        v[t] = r;
    }
}

// ------------------------------------------------------------------------------------------
// 1. centring + tolerance
// ------------------------------------------------------------------------------------------
// Column means in numpy's axis-0 order (rows added one after the other into an fp32 accumulator), X - mean in fp32,
// and the per-column variance the stop tolerance is built from (fp64).
// A block owns 64 columns.  Its 256 threads stream 128-row x 64-column tiles into LDS with 32 loads in flight per
// thread (the old thread-per-column loop had ONE dependent load in flight: 1.75 ms for 8 MB); the order-sensitive
// fp32 sum is then taken by one wave from LDS, row after row.  The fp64 moments only feed `tol`: every thread sums
// its own rows, the four row-lanes of a column are combined in a fixed order.
constexpr int KC_ROWS = 128, KC_COLS = 64;
__global__ __launch_bounds__(256) void km_center_kernel(const float* __restrict__ X, float* __restrict__ Xc, double* __restrict__ colvar,
                                                        const KmSlide* __restrict__ tab, int D) {
    __shared__ float tile[KC_ROWS][KC_COLS];
    __shared__ double part[4][KC_COLS];
    __shared__ float mean_s[KC_COLS];
    const int col = threadIdx.x & 63, rl = threadIdx.x >> 6;        // column inside the block, row-lane 0..3
    const int d = blockIdx.x * KC_COLS + col;
    const bool dok = d < D;
    const int n = tab[blockIdx.y].n;
    const size_t base = tab[blockIdx.y].row * D;
    float acc = 0.f;                                                 // wave 0 only: the fp32 column sum, rows in order
    double s64 = 0.0;
    for (int r0 = 0; r0 < n; r0 += KC_ROWS) {
        float v[KC_ROWS / 4];
#pragma unroll
        for (int u = 0; u < KC_ROWS / 4; ++u) {
            const int r = r0 + 4 * u + rl;
            v[u] = (dok && r < n) ? X[base + (size_t)r * D + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KC_ROWS / 4; ++u) { tile[4 * u + rl][col] = v[u]; s64 += (double)v[u]; }
        __syncthreads();
        if (rl == 0) {
            const int lim = min(KC_ROWS, n - r0);
            for (int r = 0; r < lim; ++r) acc += tile[r][col];
        }
        __syncthreads();
    }
    part[rl][col] = s64;
    if (rl == 0) mean_s[col] = acc / (float)n;
    __syncthreads();
    const float mean = mean_s[col];
    const double m64 = (((part[0][col] + part[1][col]) + part[2][col]) + part[3][col]) / n;
    __syncthreads();
    double q = 0.0;
    for (int r0 = 0; r0 < n; r0 += KC_ROWS) {
        float v[KC_ROWS / 4];
#pragma unroll
        for (int u = 0; u < KC_ROWS / 4; ++u) {
            const int r = r0 + 4 * u + rl;
            v[u] = (dok && r < n) ? X[base + (size_t)r * D + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KC_ROWS / 4; ++u) {
            const int r = r0 + 4 * u + rl;
            if (dok && r < n) {
                Xc[base + (size_t)r * D + d] = v[u] - mean;
                const double t = (double)v[u] - m64;
                q += t * t;
            }
        }
    }
    part[rl][col] = q;
    __syncthreads();
    if (rl == 0 && dok) colvar[(size_t)blockIdx.y * D + d] = (((part[0][col] + part[1][col]) + part[2][col]) + part[3][col]) / n;
}

__global__ void km_tol_kernel(const double* __restrict__ colvar, KmState* __restrict__ st, int D, double tol_rel) {
    __shared__ double sh[16];
    double s = 0.0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) s += colvar[(size_t)blockIdx.x * D + d];
    s = block_reduce_sum(s, sh);
    if (threadIdx.x == 0) {
        KmState& k = st[blockIdx.x];
        k.iter = 0; k.done = 0; k.strict = 0; k.n_empty = 0; k.shift = 0.0;
        k.tol = s / D * tol_rel;
    }
}

// ------------------------------------------------------------------------------------------
// 2. fp64 MFMA GEMM with fp32 operands:  C[M,N] (f64) = A[M,K] . B[N,K]^T   (batched over slides)
//    block 64x64, 4 waves x (2x2 tiles of 16x16), K-chunk 32 staged in LDS as [k][row] doubles
// ------------------------------------------------------------------------------------------
// ksl > 1: the contraction is cut into ksl slices (grid z = slide * ksl + slice), slice partials land in consecutive
// C planes and the consumer adds them in slice order (short products -- 100 centres x 1000 points -- otherwise run on
// 32 blocks with 64 dependent K steps each).
// B holds the slides' rows back to back and N is the grid's (largest) row count; slide s multiplies its own n_s rows --
// with themselves into its Gram matrix (sym), or with its M centres (A, stride sA) into its ksl planes of [M][n_s]
// behind those of the slides before it -- and blocks beyond n_s return at once.
__global__ __launch_bounds__(256) void km_dgemm_nt_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          double* __restrict__ C, int M, int N, int K, long long sA,
                                                          int ksl, int sym, const KmSlide* __restrict__ tab) {
    // sym: A == B (Gram matrix): only the blocks on and above the diagonal are computed, each also stores its mirror
    // image -- bit-exact, the products commute and the K order is the same on both sides of the diagonal
    if (sym && blockIdx.x < blockIdx.y) return;
    __shared__ double sa[32][64 + 2];
    __shared__ double sb[32][64 + 2];
    const int slide = blockIdx.z / ksl, slice = blockIdx.z - slide * ksl;
    N = tab[slide].n;
    B += tab[slide].row * K;
    if (sym) { M = N; A = B; C += tab[slide].gram; }
    else { A += (long long)slide * sA; C += (size_t)ksl * M * tab[slide].row + (size_t)slice * M * N; }
    if ((int)blockIdx.x * 64 >= N || (int)blockIdx.y * 64 >= M) return;
    const int kper = ((K + ksl - 1) / ksl + 31) / 32 * 32;
    const int k_lo = slice * kper, k_hi = min(K, k_lo + kper);
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    // loader: thread -> (row = tid / 4 within 64, k4 = tid % 4 ... two passes of 16 k each).  The next K step's rows are
    // fetched into registers before this step's MFMAs: a lone 64 x 64 block per CU otherwise spends its time waiting
    // for one round of global loads per step (the 1000 x 1000 Gram matrix: 132 -> 75 us)
    const int lrow = tid >> 2, lk = (tid & 3) * 4;
    const bool arow = m0 + lrow < M, brow = n0 + lrow < N;
    const float* ap = A + (size_t)(arow ? m0 + lrow : 0) * K;
    const float* bp = B + (size_t)(brow ? n0 + lrow : 0) * K;
    float4 va[2], vb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kk = k0 + half * 16 + lk;
            va[half] = make_float4(0.f, 0.f, 0.f, 0.f);
            vb[half] = va[half];
            if (arow && kk < k_hi) va[half] = *reinterpret_cast<const float4*>(ap + kk);
            if (brow && kk < k_hi) vb[half] = *reinterpret_cast<const float4*>(bp + kk);
        }
    };
    if (k_lo < k_hi) fetch(k_lo);
    for (int k0 = k_lo; k0 < k_hi; k0 += 32) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kr = half * 16 + lk;
            sa[kr + 0][lrow] = va[half].x; sa[kr + 1][lrow] = va[half].y; sa[kr + 2][lrow] = va[half].z; sa[kr + 3][lrow] = va[half].w;
            sb[kr + 0][lrow] = vb[half].x; sb[kr + 1][lrow] = vb[half].y; sb[kr + 2][lrow] = vb[half].z; sb[kr + 3][lrow] = vb[half].w;
        }
        __syncthreads();
        if (k0 + 32 < k_hi) fetch(k0 + 32);
#pragma unroll
        for (int ks = 0; ks < 32; ks += 4) {
            const int k = ks + (lane >> 4);
            double fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = sa[k][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = sb[k][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + i * 16 + (lane >> 4) + 4 * r;
                const int n = n0 + wn * 32 + j * 16 + (lane & 15);
                if (m < M && n < N) {
                    C[(size_t)m * N + n] = acc[i][j][r];
                    if (sym && blockIdx.x != blockIdx.y) C[(size_t)n * N + m] = acc[i][j][r];
                }
            }
}

// ------------------------------------------------------------------------------------------
// 3. k-means++ seeding: one workgroup per slide, all k-1 dependent steps inside the kernel
// ------------------------------------------------------------------------------------------
// Squared distances of the seeding step as fp32, once for all pairs: exactly pairwise.py:647-651 per element
// (d = -2 X.Y^T; d += XX; d += YY in fp64 from the Gram matrix; cast fp32; max(., 0)), row c = distances from point c.
// The seeding kernel then reads 4-byte distances (16 bytes per thread and candidate) instead of rebuilding them from
// 8-byte Gram entries inside its 99 dependent steps.
__global__ __launch_bounds__(256) void km_dist_f32_kernel(const double* __restrict__ Gall, float* __restrict__ Dall,
                                                          const KmSlide* __restrict__ tab) {
    const int c = blockIdx.x, n = tab[blockIdx.y].n;
    if (c >= n) return;
    const double* G = Gall + tab[blockIdx.y].gram;
    float* Dm = Dall + tab[blockIdx.y].gram;
    const double gcc = G[(size_t)c * n + c];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double d = -2.0 * G[(size_t)c * n + j];
        d += gcc;
        d += G[(size_t)j * n + j];
        const float f = (float)d;
        Dm[(size_t)c * n + j] = f > 0.f ? f : 0.f;
    }
}

// One step = scan -> candidates -> candidate potentials -> choice, i.e. three block-wide exchanges and ONE round of
// dependent global loads (the candidates' rows of G).  The exchanges go through LDS arrays that alternate with the
// step parity, so each costs a single barrier; the candidate distances stay in registers and the winner's are reused
// for the `closest` update (no second read of G).  Arithmetic (scan association, reduction orders) is unchanged from
// the first version of this kernel, results are bit-identical.
// Block b seeds slide list[b].  The fp64 partial sums behind fl32(potential) associate by PTS and the block size, so a
// launch covers the slides of ONE seeding class: the row of KM_SEED_LAYOUTS their row count selects.
struct KmSeedLayout { int max_rows, pts, threads; };
constexpr KmSeedLayout KM_SEED_LAYOUTS[] = {
    {1024, 4, 256},       // 4 waves x 4 points per thread: cheaper barriers and wave exchanges than 16 waves
    {2048, 2, 1024},
    {4096, 4, 1024},
};
constexpr int KM_SEED_CLASSES = sizeof(KM_SEED_LAYOUTS) / sizeof(KM_SEED_LAYOUTS[0]);
int km_seed_class(int n) {          // the first row that holds n rows; larger slides (the large route) are not seeded from a list
    int c = 0;
    while (c < KM_SEED_CLASSES - 1 && n > KM_SEED_LAYOUTS[c].max_rows) ++c;
    return c;
}

template <int PTS>   // points per thread (n <= PTS * blockDim.x)
__global__ __launch_bounds__(KM_THREADS) void km_seed_kernel(const float* __restrict__ Dall, const double* __restrict__ uniforms,
                                                             const KmSlide* __restrict__ tab, const int* __restrict__ list, int k,
                                                             int trials, int* __restrict__ seeds) {
    const int slide = list[blockIdx.x];
    const float* __restrict__ Dm = Dall + tab[slide].gram;
    const int first = tab[slide].first, n = tab[slide].n;
    int* __restrict__ out = seeds + (size_t)slide * k;
    __shared__ double sh[2][16 * KM_MAX_TRIALS];
    __shared__ int shi[2][16 * KM_MAX_TRIALS];
    __shared__ double scan_w[2][16];
    const bool vec4 = PTS == 4 && (n & 3) == 0;        // a thread's four points are one aligned 16-byte load
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;

    // thread owns the CONTIGUOUS points [tid*PTS, tid*PTS+PTS) so the scan is a plain blocked scan
    float closest[PTS];
#pragma unroll
    for (int q = 0; q < PTS; ++q) {
        const int j = tid * PTS + q;
        closest[q] = j < n ? Dm[(size_t)first * n + j] : 0.f;
    }
    float pot;
    {
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < PTS; ++q) part += (double)closest[q];
        part = wave_sum_f64(part);
        if (lane == 0) sh[1][wv] = part;
        __syncthreads();
        double r = 0.0;
        for (int i = 0; i < nw; ++i) r += sh[1][i];
        pot = (float)r;
    }
    if (tid == 0) out[0] = first;

    for (int c = 1; c < k; ++c) {
        const int par = c & 1;
        // stable_cumsum (fp64) of closest: per-thread serial, wave scan, block scan
        double run = 0.0, incl[PTS];
#pragma unroll
        for (int q = 0; q < PTS; ++q) { run += (double)closest[q]; incl[q] = run; }
        double wscan = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(wscan, o, 64);
            if (lane >= o) wscan += t;
        }
        if (lane == 63) scan_w[par][wv] = wscan;
        __syncthreads();
        double woff = 0.0;
        for (int i = 0; i < wv; ++i) woff += scan_w[par][i];
        const double excl = woff + wscan - run;          // sum of everything before this thread's points
        // candidates: searchsorted(cumsum, u * pot, side='left') = #{cum < value}, clipped to n-1 (all trials at once)
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            if (t < trials) {
                const double rv = uniforms[(size_t)(c - 1) * trials + t] * (double)pot;
                int cnt = 0;
#pragma unroll
                for (int q = 0; q < PTS; ++q)
                    cnt += __popcll(__ballot(tid * PTS + q < n && excl + incl[q] < rv));
                if (lane == 0) shi[par][wv * KM_MAX_TRIALS + t] = cnt;
            }
        }
        __syncthreads();
        int cand[KM_MAX_TRIALS];
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            int r = 0;
            if (t < trials)
                for (int i = 0; i < nw; ++i) r += shi[par][i * KM_MAX_TRIALS + t];
            cand[t] = r > n - 1 ? n - 1 : r;
        }
        // distances to the candidates (one round of loads for all trials), potentials
        float dc[KM_MAX_TRIALS][PTS];
        double p[KM_MAX_TRIALS];
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            if (t < trials) {
                const float* row = Dm + (size_t)cand[t] * n;
                if constexpr (PTS == 4) {
                    if (vec4 && tid * 4 < n) {
                        const float4 v = *reinterpret_cast<const float4*>(row + tid * 4);
                        dc[t][0] = v.x; dc[t][1] = v.y; dc[t][2] = v.z; dc[t][3] = v.w;
                    } else {
#pragma unroll
                        for (int q = 0; q < PTS; ++q) dc[t][q] = tid * PTS + q < n ? row[tid * PTS + q] : 0.f;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < PTS; ++q) dc[t][q] = tid * PTS + q < n ? row[tid * PTS + q] : 0.f;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            p[t] = 0.0;
            if (t < trials) {
#pragma unroll
                for (int q = 0; q < PTS; ++q)
                    if (tid * PTS + q < n) p[t] += (double)fminf(closest[q], dc[t][q]);
            } else {
#pragma unroll
                for (int q = 0; q < PTS; ++q) dc[t][q] = 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) p[t] = wave_sum_f64(p[t]);
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < KM_MAX_TRIALS; ++t) sh[par][wv * KM_MAX_TRIALS + t] = p[t];
        }
        __syncthreads();
        float best_pot = 0.f;
        int best_t = 0;
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            if (t < trials) {
                double r = 0.0;
                for (int i = 0; i < nw; ++i) r += sh[par][i * KM_MAX_TRIALS + t];
                const float pt = (float)r;
                if (t == 0 || pt < best_pot) { best_pot = pt; best_t = t; }     // np.argmin: first minimum
            }
        }
        int chosen = cand[0];
#pragma unroll
        for (int t = 1; t < KM_MAX_TRIALS; ++t)
            if (t == best_t) chosen = cand[t];
        pot = best_pot;
#pragma unroll
        for (int q = 0; q < PTS; ++q) {
            float f = dc[0][q];
#pragma unroll
            for (int t = 1; t < KM_MAX_TRIALS; ++t)
                if (t == best_t) f = dc[t][q];
            if (tid * PTS + q < n) closest[q] = fminf(closest[q], f);
        }
        if (tid == 0) out[c] = chosen;
    }
}

__global__ void km_gather_centers_kernel(const float* __restrict__ Xc, const int* __restrict__ seeds, float* __restrict__ centers,
                                         const KmSlide* __restrict__ tab, int D, int k) {
    const int c = blockIdx.x, s = blockIdx.y;
    const int src = seeds[(size_t)s * k + c];
    for (int d = threadIdx.x; d < D; d += blockDim.x)
        centers[((size_t)s * k + c) * D + d] = Xc[(tab[s].row + src) * D + d];
}

// ------------------------------------------------------------------------------------------
// 4. Lloyd iteration pieces (every kernel returns at once for slides that are done)
// ------------------------------------------------------------------------------------------
// |c|^2 in fp64, one wave per centre (lanes stride the row, butterfly sum): its own launch, because inside the assign
// kernel every block recomputed all k norms with 25 dependent row walks per wave (0.25 ms of a 0.3 ms kernel)
__global__ __launch_bounds__(64) void km_center_norms_kernel(const float* __restrict__ centers, double* __restrict__ cnorm,
                                                             const KmState* __restrict__ st, int D, int k, int force) {
    const int c = blockIdx.x, s = blockIdx.y;
    if (st[s].done && !force) return;
    const float* cr = centers + ((size_t)s * k + c) * D;
    double a = 0.0;
    int d = threadIdx.x;
    for (; d + 7 * 64 < D; d += 8 * 64) {          // eight loads in flight, added in the same (ascending d) order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = cr[d + 64 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += (double)v[u] * (double)v[u];
    }
    for (; d < D; d += 64) a += (double)cr[d] * (double)cr[d];
    a = wave_sum_f64(a);
    if (threadIdx.x == 0) cnorm[(size_t)s * k + c] = a;
}

// labels[j] = argmin_c (|c|^2 - 2 x_j.c), strict '<' (first minimum); dots from the fp64 GEMM as ksl planes of
// [k centres][n points] (a thread walks the centres of ITS point: consecutive threads read consecutive doubles)
__global__ __launch_bounds__(1024) void km_assign_kernel(const double* __restrict__ dots, const double* __restrict__ cnorm, int* __restrict__ labels,
                                                         const KmState* __restrict__ st, const KmSlide* __restrict__ tab, int D, int k,
                                                         int force, int ksl) {
    // block = 64 points x 16 centre groups (wave g walks centres [g*k/16, (g+1)*k/16) of its 64 points, all of their
    // slice loads in flight together); the partial minima are merged in centre order, which keeps the first minimum
    constexpr int G = 16, CB = 7;
    __shared__ double cn[KM_MAX_K];
    __shared__ double bval[G][64];
    __shared__ int blab[G][64];
    const int s = blockIdx.y;
    if (st[s].done && !force) return;
    const int n = tab[s].n;
    if ((int)blockIdx.x * 64 >= n) return;
    for (int c = threadIdx.x; c < k; c += blockDim.x) cn[c] = cnorm[(size_t)s * k + c];
    __syncthreads();
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int c_lo = g * k / G, c_hi = (g + 1) * k / G;
    const size_t plane = (size_t)k * n;
    const double* dr = dots + (size_t)ksl * k * tab[s].row + (j < n ? j : 0);
    double best = 0.0;
    int lab = -1;
    for (int c0 = c_lo; c0 < c_hi; c0 += CB) {
        double dot[CB];
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            const int c = c0 + u < c_hi ? c0 + u : c_hi - 1;
            double a = dr[(size_t)c * n];
            for (int q = 1; q < ksl; ++q) a += dr[q * plane + (size_t)c * n];
            dot[u] = a;
        }
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            const int c = c0 + u;
            if (c < c_hi) {
                const double v = cn[c] - 2.0 * dot[u];
                if (lab < 0 || v < best) { best = v; lab = c; }
            }
        }
    }
    bval[g][lane] = best;
    blab[g][lane] = lab;
    __syncthreads();
    if (g == 0 && j < n) {
        double b = bval[0][lane];
        int l = blab[0][lane];
#pragma unroll
        for (int q = 1; q < G; ++q)
            if (blab[q][lane] >= 0 && (l < 0 || bval[q][lane] < b)) { b = bval[q][lane]; l = blab[q][lane]; }
        labels[tab[s].row + j] = l;
    }
}

// counting sort of point ids by label, stable in the point index: members[off[c] .. off[c+1])
// (n <= 4096: one workgroup, labels in LDS; larger slides: km_lg_hist / km_lg_offsets / km_lg_scatter)
__global__ __launch_bounds__(KM_THREADS) void km_members_kernel(const int* __restrict__ labels, int* __restrict__ members,
                                                                int* __restrict__ offsets, const KmState* __restrict__ st,
                                                                const KmSlide* __restrict__ tab, int k, int force) {
    __shared__ int slab[4096];
    __shared__ int soff[KM_MAX_K + 1];
    const int s = blockIdx.x;
    if (st[s].done && !force) return;
    const int n = tab[s].n;
    const size_t r0 = tab[s].row;
    for (int j = threadIdx.x; j < n; j += blockDim.x) slab[j] = labels[r0 + j];
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += blockDim.x) {
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += slab[j] == c;
        soff[c + 1] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        soff[0] = 0;
        for (int c = 0; c < k; ++c) soff[c + 1] += soff[c];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int lab = slab[j];
        int rank = 0;
        for (int i = 0; i < j; ++i) rank += slab[i] == lab;
        members[r0 + soff[lab] + rank] = j;
    }
    for (int c = threadIdx.x; c <= k; c += blockDim.x) offsets[(size_t)s * (k + 1) + c] = soff[c];
}

// sums[c, d] = sum over members (index order) of Xc in fp64
__global__ void km_sums_kernel(const float* __restrict__ Xc, const int* __restrict__ members, const int* __restrict__ offsets,
                               double* __restrict__ sums, const KmState* __restrict__ st, const KmSlide* __restrict__ tab, int D, int k) {
    const int c = blockIdx.x, s = blockIdx.y;
    if (st[s].done) return;
    const int lo = offsets[(size_t)s * (k + 1) + c], hi = offsets[(size_t)s * (k + 1) + c + 1];
    const size_t r0 = tab[s].row;
    const int* mem = members + r0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        double a = 0.0;
        int i = lo;
        for (; i + 8 <= hi; i += 8) {              // eight gathered rows in flight, added in member (= index) order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = Xc[(r0 + mem[i + u]) * D + d];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)v[u];
        }
        for (; i < hi; ++i) a += (double)Xc[(r0 + mem[i]) * D + d];
        sums[((size_t)s * k + c) * D + d] = a;
    }
}

// _relocate_empty_clusters_dense (_k_means_common.pyx:167-211), one workgroup per slide; rare path
__global__ __launch_bounds__(KM_THREADS) void km_relocate_kernel(const float* __restrict__ Xc, const float* __restrict__ centers,
                                                                 const int* __restrict__ labels, int* __restrict__ offsets,
                                                                 double* __restrict__ sums, double* __restrict__ weights,
                                                                 double* __restrict__ dist_ws, const KmState* __restrict__ st,
                                                                 const KmSlide* __restrict__ tab, int D, int k) {
    __shared__ int empty[KM_MAX_K];
    __shared__ int n_empty;
    __shared__ int far_idx;
    const int s = blockIdx.x;
    if (st[s].done) return;
    const int n = tab[s].n;
    const size_t r0 = tab[s].row;
    const int* off = offsets + (size_t)s * (k + 1);
    double* w = weights + (size_t)s * k;
    for (int c = threadIdx.x; c < k; c += blockDim.x) w[c] = (double)(off[c + 1] - off[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        int e = 0;
        for (int c = 0; c < k; ++c)
            if (w[c] == 0.0) empty[e++] = c;
        n_empty = e;
    }
    __syncthreads();
    if (n_empty == 0) return;
    // distances of every point to its (old) centre: ((X - centers_old[labels])**2).sum(axis=1)
    double* dist = dist_ws + r0;
    for (int j = threadIdx.x >> 6; j < n; j += blockDim.x >> 6) {
        const float* xr = Xc + (r0 + j) * D;
        const float* cr = centers + ((size_t)s * k + labels[r0 + j]) * D;
        double a = 0.0;
        for (int d = threadIdx.x & 63; d < D; d += 64) { const float t = xr[d] - cr[d]; a += (double)(t * t); }
        a = wave_sum_f64(a);
        if ((threadIdx.x & 63) == 0) dist[j] = a;
    }
    __syncthreads();
    for (int e = 0; e < n_empty; ++e) {
        if (threadIdx.x == 0) {          // farthest remaining point (descending distance, ties by index)
            int bi = -1; double bd = -1.0;
            for (int j = 0; j < n; ++j)
                if (dist[j] > bd) { bd = dist[j]; bi = j; }
            // np.max(distances) == 0 is asked ONCE, of the farthest point of all: with fewer points off their centres than
            // empty clusters the remaining clusters still take points at distance 0, lowest index first
            far_idx = (e > 0 || bd > 0.0) ? bi : -1;
            if (bi >= 0) dist[bi] = -2.0;
        }
        __syncthreads();
        const int fi = far_idx;
        if (fi < 0) break;               // np.max(distances) == 0: relocation is pointless
        const int new_id = empty[e], old_id = labels[r0 + fi];
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            const double x = (double)Xc[(r0 + fi) * D + d];
            sums[((size_t)s * k + old_id) * D + d] -= x;
            sums[((size_t)s * k + new_id) * D + d] = x;
        }
        __syncthreads();
        if (threadIdx.x == 0) { w[new_id] = 1.0; w[old_id] -= 1.0; }
        __syncthreads();
    }
}

// _average_centers + _center_shift: one block per (cluster, slide) writes the new centre row into the OTHER centre
// buffer (a cluster left empty copies the heaviest cluster's new row, so rows cannot be updated in place) and its
// share of the squared shift; slides that are done copy their rows through, so both buffers stay valid for them.
__global__ __launch_bounds__(256) void km_update_centers_kernel(const float* __restrict__ centers, float* __restrict__ centers_new,
                                                                const double* __restrict__ sums, const double* __restrict__ weights,
                                                                double* __restrict__ shift_part, const KmState* __restrict__ st,
                                                                int D, int k) {
    __shared__ double sh[16];
    __shared__ int amax_s;
    const int c = blockIdx.x, s = blockIdx.y;
    const float* old_row = centers + ((size_t)s * k + c) * D;
    float* new_row = centers_new + ((size_t)s * k + c) * D;
    if (st[s].done) {
        for (int d = threadIdx.x; d < D; d += blockDim.x) new_row[d] = old_row[d];
        return;
    }
    const double* w = weights + (size_t)s * k;
    if (threadIdx.x == 0) {
        int a = 0;
        for (int i = 1; i < k; ++i)
            if (w[i] > w[a]) a = i;      // np.argmax: first maximum
        amax_s = a;
    }
    __syncthreads();
    const int src = w[c] > 0.0 ? c : amax_s;
    const double ws = w[src];
    const double* srow = sums + ((size_t)s * k + src) * D;
    double shift = 0.0;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const float nv = (float)(srow[d] / ws);
        const double df = (double)nv - (double)old_row[d];
        shift += df * df;
        new_row[d] = nv;
    }
    shift = block_reduce_sum(shift, sh);
    if (threadIdx.x == 0) shift_part[(size_t)s * k + c] = shift;
}

// the stop rule of _kmeans_single_lloyd; one workgroup per slide
__global__ __launch_bounds__(KM_THREADS) void km_finish_iter_kernel(const double* __restrict__ shift_part, const int* __restrict__ labels,
                                                                    int* __restrict__ labels_old, KmState* __restrict__ st,
                                                                    const KmSlide* __restrict__ tab, int k, int max_iter) {
    __shared__ int shi[16];
    const int s = blockIdx.x;
    if (st[s].done) return;
    const int n = tab[s].n;
    const size_t r0 = tab[s].row;
    int diff = 0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int l = labels[r0 + j];
        diff += l != labels_old[r0 + j];
        labels_old[r0 + j] = l;
    }
    diff = block_reduce_sum_int(diff, shi);
    if (threadIdx.x == 0) {
        double shift = 0.0;
        for (int c = 0; c < k; ++c) shift += shift_part[(size_t)s * k + c];      // cluster order
        KmState& ks = st[s];
        ks.iter += 1;
        ks.shift = shift;
        if (diff == 0) { ks.strict = 1; ks.done = 1; }
        else if (shift <= ks.tol) ks.done = 1;
        else if (ks.iter >= max_iter) ks.done = 1;
    }
}

__global__ void km_restore_strict_kernel(int* __restrict__ labels, const int* __restrict__ labels_old, const KmState* __restrict__ st,
                                         const KmSlide* __restrict__ tab) {
    const int s = blockIdx.y;
    if (!st[s].strict) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < tab[s].n) labels[tab[s].row + j] = labels_old[tab[s].row + j];
}

__global__ void km_count_done_kernel(const KmState* __restrict__ st, int S, int* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int d = 0, q = 0;
        for (int s = 0; s < S; ++s) { d += st[s].done; q += st[s].strict; }
        out[0] = d;
        out[1] = q;
    }
}

__global__ void km_report_kernel(const KmState* __restrict__ st, int S, int* __restrict__ n_iter) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && n_iter) n_iter[s] = st[s].iter;
}

// kmean_features.py:99-105: np.mean(features[labels == c], axis=0): fp32 adds in index order, / count
__global__ void km_cluster_means_kernel(const float* __restrict__ X, const int* __restrict__ members, const int* __restrict__ offsets,
                                        float* __restrict__ out, const KmSlide* __restrict__ tab, int D, int k) {
    const int c = blockIdx.x, s = blockIdx.y;
    const int lo = offsets[(size_t)s * (k + 1) + c], hi = offsets[(size_t)s * (k + 1) + c + 1];
    const size_t r0 = tab[s].row;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float a = 0.f;
        for (int i = lo; i < hi; ++i) a += X[(r0 + members[r0 + i]) * D + d];
        out[((size_t)s * k + c) * D + d] = a / (float)(hi - lo);      // empty cluster -> 0/0 = NaN like numpy
    }
}

// ------------------------------------------------------------------------------------------
// 5. slides of more than 4096 points: seeding without the Gram matrix, member lists for any n
// ------------------------------------------------------------------------------------------
// The Gram route holds n^2 distances and all points of a slide in ONE workgroup's registers.  Here a seeding step only
// forms the distances of its <= 8 candidates to all n points ([T, n] = Xc[cand] . Xc^T on the fp64 MFMA, 16-row M tile,
// candidate rows gathered through device-side indices), `closest` lives in global memory, and a step is three plain
// dependent launches: pick (scan + candidate search per 1024-point chunk), dist (product + distance epilogue +
// per-tile potentials), choose (potentials -> winner -> `closest` update + chunk sums).  Every reduction has a fixed
// association that depends on n alone (64-point tiles, 1024-point chunks, tiles / chunks combined in index order).
// The dot products run through the MFMA in the K order of km_dgemm_nt_kernel (one accumulator, k ascending in steps
// of 4), and the row norms are the diagonal of the same product, so x.x, x.c and c.c of two identical rows are the
// same bits and a point's distance to itself or to a duplicate is exactly 0, as on the Gram route.
constexpr int KM_LG_MAX_N = SQ_KMEANS_LARGE_MAX_SAMPLES;      // 65536, the stated bound of sq_kmeans_fit_large
constexpr int KM_LG_CHUNK = 1024;                             // points per scan / sort chunk (one workgroup)
constexpr int KM_LG_MAX_CHUNKS = KM_LG_MAX_N / KM_LG_CHUNK;   // 64
constexpr int KM_LG_TILE = 64;                                // points per block of the distance product
constexpr int KM_LG_MAX_TILES = KM_LG_MAX_N / KM_LG_TILE;     // 1024 = one partial per thread of the choose kernel

struct KmLgBufs {         // per call (one slide), device memory
    double* norms;        // [n] |x|^2 of the centred rows (fp64, MFMA association)
    float* closest;       // [n] squared distance to the nearest chosen centre
    float* distc;         // [KM_MAX_TRIALS][n] the step's candidate distances
    double* part;         // [KM_MAX_TRIALS][KM_LG_MAX_TILES] per-tile potentials of the candidates
    double* chunk_sum;    // [KM_LG_MAX_CHUNKS] sum of `closest` per chunk
    int* cnt;             // [KM_MAX_TRIALS][KM_LG_MAX_CHUNKS] #{cumsum < u * pot} per chunk
    int* cand;            // [KM_MAX_TRIALS] the step's candidates
    float* pot;           // current potential
    int* hist;            // [KM_LG_MAX_CHUNKS][KM_MAX_K] per-chunk label histogram, then per-chunk start inside the cluster
};

// MODE 0: norms[j] = x_j . x_j (diagonal of the 16 x 16 self product of each row group).
// MODE 1: distc[t][j] = fl32(max(0, (-2 x_cand[t] . x_j + |x_cand[t]|^2) + |x_j|^2)) and the tile's share of every
//         candidate's potential sum_j min(closest[j], distc[t][j]) (fp64; init: sum_j distc[0][j], the first centre).
// block = 64 points (4 waves x 16) x 16 candidate rows (rows >= trials are zero).  A block walks the whole contraction
// on one accumulator per wave, so what it waits for is the round trip of its loads: K goes in chunks of 128 (16 rounds at
// D = 2048, ten 16-byte loads per thread in flight, issued before the 32 MFMAs of the chunk in hand), staged in LDS as
// fp32 rows (k contiguous, +4 floats of padding: the MFMA operand reads hit 64 different banks) and widened on the way out.
constexpr int KM_LG_KC = 128;
template <int MODE>
__global__ __launch_bounds__(256) void km_lg_rows_kernel(const float* __restrict__ Xc, double* __restrict__ norms,
                                                         const int* __restrict__ cnt, int* __restrict__ cand_out,
                                                         const float* __restrict__ closest, float* __restrict__ distc,
                                                         double* __restrict__ part, int n, int D, int trials, int nchunks,
                                                         int init, int first) {
    __shared__ __attribute__((aligned(16))) float sa[MODE ? 16 : 1][KM_LG_KC + 4];
    __shared__ __attribute__((aligned(16))) float sb[KM_LG_TILE][KM_LG_KC + 4];
    __shared__ int cand_s[16];
    __shared__ double psh[4][KM_MAX_TRIALS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * KM_LG_TILE;
    if (MODE) {
        if (tid < 16) {
            int c = 0;
            if (tid < trials) {
                if (init) c = first;
                else {
                    for (int b = 0; b < nchunks; ++b) c += cnt[tid * KM_LG_MAX_CHUNKS + b];      // searchsorted(side='left')
                    c = c > n - 1 ? n - 1 : c;
                }
                if (blockIdx.x == 0) cand_out[tid] = c;
            }
            cand_s[tid] = c;
        }
        __syncthreads();
    }
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    // loader: float4 number tid + 256 u of the chunk, 32 of them per row: a wave reads two rows' 512 contiguous bytes
    const int lk = (tid & 31) * 4, lr = tid >> 5;               // row lr + 8 u
    const float* bp[8];
    bool bok[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        bok[u] = j0 + lr + 8 * u < n;
        bp[u] = Xc + (size_t)(bok[u] ? j0 + lr + 8 * u : 0) * D + lk;
    }
    const float* ap[2];
    bool aok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        aok[u] = MODE && lr + 8 * u < trials;
        ap[u] = Xc + (size_t)(aok[u] ? cand_s[lr + 8 * u] : 0) * D + lk;
    }
    float4 va[2], vb[8];
    auto fetch = [&](int k0) {
        const bool kok = k0 + lk < D;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            va[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (aok[u] && kok) va[u] = *reinterpret_cast<const float4*>(ap[u] + k0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            vb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bok[u] && kok) vb[u] = *reinterpret_cast<const float4*>(bp[u] + k0);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += KM_LG_KC) {
        if (MODE) {
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<float4*>(&sa[lr + 8 * u][lk]) = va[u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(&sb[lr + 8 * u][lk]) = vb[u];
        __syncthreads();
        if (k0 + KM_LG_KC < D) fetch(k0 + KM_LG_KC);
        const int klim = min(KM_LG_KC, D - k0);                  // D % 4 == 0: whole MFMA steps, k ascending as in km_dgemm_nt_kernel
        auto step = [&](int ks) {
            const int kq = ks + (lane >> 4);
            const double fb = (double)sb[wave * 16 + (lane & 15)][kq];
            const double fa = MODE ? (double)sa[lane & 15][kq] : fb;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc, 0, 0, 0);
        };
        int ks = 0;
        for (; ks + 32 <= klim; ks += 32) {
#pragma unroll
            for (int q = 0; q < 32; q += 4) step(ks + q);
        }
        for (; ks < klim; ks += 4) step(ks);
        __syncthreads();
    }
    // f64 C/D layout: col (point) = lane & 15, row (candidate) = (lane >> 4) + 4 * reg
    const int j = j0 + wave * 16 + (lane & 15);
    if (!MODE) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if ((lane >> 4) + 4 * r == (lane & 15) && j < n) norms[j] = acc[r];
        return;
    }
    const double nj = j < n ? norms[j] : 0.0;
    const float cl = (j < n && !init) ? closest[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {                                // candidate rows 0..7 (KM_MAX_TRIALS)
        const int t = (lane >> 4) + 4 * r;
        double pv = 0.0;
        if (t < trials && j < n) {
            double d = -2.0 * acc[r];
            d += norms[cand_s[t]];
            d += nj;
            float f = (float)d;
            f = f > 0.f ? f : 0.f;
            distc[(size_t)t * n + j] = f;
            pv = (double)(init ? f : fminf(cl, f));
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) pv += __shfl_xor(pv, o, 64);      // the 16 points of this wave, fixed butterfly
        if ((lane & 15) == 0) psh[wave][t] = pv;
    }
    __syncthreads();
    if (tid < trials) part[(size_t)tid * KM_LG_MAX_TILES + blockIdx.x] = ((psh[0][tid] + psh[1][tid]) + psh[2][tid]) + psh[3][tid];
}

// stable_cumsum (fp64) of `closest` over chunk b (chunk sums added in chunk order in front of a blocked scan) and, for
// every trial, how many of the chunk's points have cumsum < u * pot
__global__ __launch_bounds__(KM_LG_CHUNK) void km_lg_pick_kernel(const float* __restrict__ closest, const double* __restrict__ chunk_sum,
                                                                 const float* __restrict__ pot, const double* __restrict__ uniforms,
                                                                 int* __restrict__ cnt, int n, int trials) {
    __shared__ double scan_w[16];
    __shared__ int shi[16][KM_MAX_TRIALS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = blockIdx.x * KM_LG_CHUNK + tid;
    double base = 0.0;
    for (int b = 0; b < (int)blockIdx.x; ++b) base += chunk_sum[b];
    const double v = j < n ? (double)closest[j] : 0.0;
    double wscan = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(wscan, o, 64);
        if (lane >= o) wscan += t;
    }
    if (lane == 63) scan_w[wv] = wscan;
    __syncthreads();
    double woff = base;
    for (int i = 0; i < wv; ++i) woff += scan_w[i];
    const double cum = woff + wscan;
    const double p = (double)pot[0];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) {
        if (t < trials) {
            const double rv = uniforms[t] * p;
            const int c = __popcll(__ballot(j < n && cum < rv));
            if (lane == 0) shi[wv][t] = c;
        }
    }
    __syncthreads();
    if (tid < trials) {
        int r = 0;
        for (int i = 0; i < 16; ++i) r += shi[i][tid];
        cnt[tid * KM_LG_MAX_CHUNKS + blockIdx.x] = r;
    }
}

// potentials fl32(sum_fp64) of the candidates (tile shares, one per thread, reduced in a fixed tree), np.argmin
// (first minimum); then closest = min(closest, winner's distances) for this block's chunk and the chunk's new sum.
// Every block takes the same decision from the same numbers; block 0 records it.
__global__ __launch_bounds__(KM_LG_CHUNK) void km_lg_choose_kernel(const double* __restrict__ part, const float* __restrict__ distc,
                                                                   const int* __restrict__ cand, float* __restrict__ closest,
                                                                   double* __restrict__ chunk_sum, float* __restrict__ pot,
                                                                   int* __restrict__ seed_out, int n, int trials, int ntiles, int init) {
    __shared__ double sh[16 * KM_MAX_TRIALS];
    const int tid = threadIdx.x;
    double p[KM_MAX_TRIALS];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) p[t] = (t < trials && tid < ntiles) ? part[(size_t)t * KM_LG_MAX_TILES + tid] : 0.0;
    block_reduce_sum_n<KM_MAX_TRIALS>(p, sh);
    float best_pot = 0.f;
    int best_t = 0;
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) {
        if (t < trials) {
            const float pt = (float)p[t];
            if (t == 0 || pt < best_pot) { best_pot = pt; best_t = t; }
        }
    }
    const int j = blockIdx.x * KM_LG_CHUNK + tid;
    double c = 0.0;
    if (j < n) {
        const float f = distc[(size_t)best_t * n + j];
        const float m = init ? f : fminf(closest[j], f);
        closest[j] = m;
        c = (double)m;
    }
    c = block_reduce_sum(c, sh);
    if (tid == 0) {
        chunk_sum[blockIdx.x] = c;
        if (blockIdx.x == 0) { pot[0] = best_pot; seed_out[0] = cand[best_t]; }
    }
}

// Member lists for any n: a counting sort of point ids by label, stable in the point index, in three launches --
// per-chunk histograms; a scan over the chunks in chunk order (per cluster) and over the clusters; scatter with the
// rank inside the chunk.  Gives exactly the members / offsets of km_members_kernel.
__global__ __launch_bounds__(KM_LG_CHUNK) void km_lg_hist_kernel(const int* __restrict__ labels, int* __restrict__ hist,
                                                                 const KmState* __restrict__ st, int n, int k, int force) {
    __shared__ int h[KM_MAX_K];
    if (st[0].done && !force) return;
    if (threadIdx.x < KM_MAX_K) h[threadIdx.x] = 0;
    __syncthreads();
    const int j = blockIdx.x * KM_LG_CHUNK + threadIdx.x;
    if (j < n) {
        const int lab = labels[j];
        if ((unsigned)lab < (unsigned)k) atomicAdd(&h[lab], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < k) hist[blockIdx.x * KM_MAX_K + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(KM_MAX_K) void km_lg_offsets_kernel(int* __restrict__ hist, int* __restrict__ offsets,
                                                                 const KmState* __restrict__ st, int nchunks, int k, int force) {
    __shared__ int soff[KM_MAX_K + 1];
    if (st[0].done && !force) return;
    const int c = threadIdx.x;
    if (c < k) {
        int run = 0;
        for (int b = 0; b < nchunks; ++b) {
            const int t = hist[b * KM_MAX_K + c];
            hist[b * KM_MAX_K + c] = run;          // members of cluster c in earlier chunks
            run += t;
        }
        soff[c + 1] = run;
    }
    __syncthreads();
    if (c == 0) {
        soff[0] = 0;
        for (int i = 0; i < k; ++i) soff[i + 1] += soff[i];
    }
    __syncthreads();
    for (int i = c; i <= k; i += blockDim.x) offsets[i] = soff[i];
}

__global__ __launch_bounds__(KM_LG_CHUNK) void km_lg_scatter_kernel(const int* __restrict__ labels, const int* __restrict__ hist,
                                                                    const int* __restrict__ offsets, int* __restrict__ members,
                                                                    const KmState* __restrict__ st, int n, int k, int force) {
    __shared__ int slab[KM_LG_CHUNK];
    if (st[0].done && !force) return;
    const int tid = threadIdx.x;
    const int j = blockIdx.x * KM_LG_CHUNK + tid;
    const int lab = j < n ? labels[j] : -1;
    slab[tid] = lab;
    __syncthreads();
    if ((unsigned)lab >= (unsigned)k) return;
    int rank = 0;
    for (int i = 0; i < tid; ++i) rank += slab[i] == lab;
    const int pos = offsets[lab] + hist[blockIdx.x * KM_MAX_K + lab] + rank;
    if (pos < n) members[pos] = j;
}


struct KmBufs {
    float* Xc; double* colvar; double* G; float* centers; float* centers2; double* shift_part; double* dots; double* sums; double* weights; double* dist;
    int* seeds; int* labels_old; int* members; int* offsets; int* done_count; KmState* st;
    float* dist32;
    KmSlide* tab; int* cls_list;      // the slide table [S] and the slide indices by seeding class [S], one block
    size_t bytes;
};

// The slides of a call as its entry names them: slide s has ns[s * stride] rows and first centre firsts[s * stride].
// stride 0: S equal slides (sq_kmeans_fit), or the one of sq_kmeans_fit_large; stride 1: the lists of sq_kmeans_fit_ragged.
struct KmCounts {
    int S;
    const int32_t* ns;
    const int32_t* firsts;
    int stride;
    int n(int s) const { return ns[(size_t)s * stride]; }
    int first(int s) const { return firsts[(size_t)s * stride]; }
};

struct KmExtents {
    size_t rows, gram;                // rows and n x n elements (each slide's rounded up to 4) of all slides
    int n_max;                        // the largest slide: sizes the grids
    int cls_n[KM_SEED_CLASSES];       // slides per seeding class
};

// The one walk over the counts: the extents and, with `host`, the block the device reads -- the slide table and behind
// it the slide indices grouped by seeding class, in slide order inside a class.
KmExtents km_walk(const KmCounts& c, std::vector<char>* host) {
    KmExtents e{};
    KmSlide* tab = nullptr;
    if (host) {
        host->resize((size_t)c.S * (sizeof(KmSlide) + 4));
        tab = (KmSlide*)host->data();
    }
    for (int s = 0; s < c.S; ++s) {
        const int n = c.n(s);
        if (tab) tab[s] = KmSlide{n, c.first(s), e.rows, e.gram};
        e.rows += (size_t)n;
        e.gram += km_gram_elems(n);
        if (n > e.n_max) e.n_max = n;
        ++e.cls_n[km_seed_class(n)];
    }
    if (tab) {
        int* list = (int*)(tab + c.S);
        int fill[KM_SEED_CLASSES];
        for (int q = 0, at = 0; q < KM_SEED_CLASSES; at += e.cls_n[q++]) fill[q] = at;
        for (int s = 0; s < c.S; ++s) list[fill[km_seed_class(tab[s].n)]++] = s;
    }
    return e;
}

// The workspace of S slides of the extents e.
// lg != nullptr: the large-slide route (no Gram matrix, no n^2 distances; its own seeding / sort buffers behind the rest).
void km_carve(int S, const KmExtents& e, int D, int k, char* base, KmBufs* o, KmLgBufs* lg) {
    const size_t rows = e.rows, gram = e.gram;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = sq_align_up(off, 256); char* p = base ? base + off : nullptr; off += bytes; return (void*)p; };
    o->Xc = (float*)take(rows * D * 4);
    o->colvar = (double*)take((size_t)S * D * 8);
    o->G = (double*)take(lg ? 0 : gram * 8);
    o->centers = (float*)take((size_t)S * k * D * 4);
    o->centers2 = (float*)take((size_t)S * k * D * 4);
    o->shift_part = (double*)take((size_t)S * k * 8 * 2);      // [S][k] shift shares, then [S][k] centre norms
    o->dots = (double*)take((size_t)KM_DOT_SLICES * rows * k * 8);
    o->sums = (double*)take((size_t)S * k * D * 8);
    o->weights = (double*)take((size_t)S * k * 8);
    o->dist = (double*)take(rows * 8);
    o->seeds = (int*)take((size_t)S * k * 4);
    o->labels_old = (int*)take(rows * 4);
    o->members = (int*)take(rows * 4);
    o->offsets = (int*)take((size_t)S * (k + 1) * 4);
    o->done_count = (int*)take(256);
    o->st = (KmState*)take((size_t)S * sizeof(KmState));
    o->dist32 = (float*)take(lg ? 0 : gram * 4);
    if (lg) {
        const size_t n = rows;          // one slide
        lg->norms = (double*)take(n * 8);
        lg->closest = (float*)take(n * 4);
        lg->distc = (float*)take((size_t)KM_MAX_TRIALS * n * 4);
        lg->part = (double*)take((size_t)KM_MAX_TRIALS * KM_LG_MAX_TILES * 8);
        lg->chunk_sum = (double*)take((size_t)KM_LG_MAX_CHUNKS * 8);
        lg->cnt = (int*)take((size_t)KM_MAX_TRIALS * KM_LG_MAX_CHUNKS * 4);
        lg->cand = (int*)take(KM_MAX_TRIALS * 4);
        lg->pot = (float*)take(4);
        lg->hist = (int*)take((size_t)KM_LG_MAX_CHUNKS * KM_MAX_K * 4);
    }
    o->tab = (KmSlide*)take((size_t)S * (sizeof(KmSlide) + 4));
    o->cls_list = base ? (int*)(o->tab + S) : nullptr;
    o->bytes = sq_align_up(off, 256);
}

// The Lloyd loop, the final E-step and the cluster means: expects the slide table in b.tab, the centred data, the
// tolerance state, the seeded centres in b.centers and labels_old = -1.  n, the largest slide's row count, sizes the
// grids: blocks beyond their own slide's rows return at once.  lg == nullptr: member lists by km_members_kernel
// (n <= 4096, any S); otherwise by the three-launch counting sort (any n, S == 1).
int km_lloyd_and_means(const float* X, int S, int n, int D, int k, int max_iter, int32_t* labels, float* cluster_features,
                       int32_t* n_iter, float* final_centers, const KmBufs& b, const KmLgBufs* lg, hipStream_t st) {
    const KmSlide* tab = b.tab;
    auto members = [&](int force) -> int {
        if (!lg) {
            hipLaunchKernelGGL(km_members_kernel, dim3(S), dim3(KM_THREADS), 0, st, labels, b.members, b.offsets, b.st, tab, k, force);
            SQ_LAUNCH_CHECK();
            return SQ_OK;
        }
        const int nchunks = (n + KM_LG_CHUNK - 1) / KM_LG_CHUNK;
        hipLaunchKernelGGL(km_lg_hist_kernel, dim3(nchunks), dim3(KM_LG_CHUNK), 0, st, labels, lg->hist, b.st, n, k, force);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_lg_offsets_kernel, dim3(1), dim3(KM_MAX_K), 0, st, lg->hist, b.offsets, b.st, nchunks, k, force);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_lg_scatter_kernel, dim3(nchunks), dim3(KM_LG_CHUNK), 0, st, labels, lg->hist, b.offsets, b.members, b.st, n, k, force);
        SQ_LAUNCH_CHECK();
        return SQ_OK;
    };
    float* cur = b.centers;          // centres of the iteration in flight; the update writes the other buffer
    float* nxt = b.centers2;
    const int ksl = D >= 32 * KM_DOT_SLICES ? KM_DOT_SLICES : 1;
    auto e_step = [&](int force) -> int {
        // dots[slice][centre][point] = centres . points (fp64), K sliced so that the launch fills the chip
        hipLaunchKernelGGL(km_dgemm_nt_kernel, dim3((n + 63) / 64, (k + 63) / 64, S * ksl), dim3(256), 0, st, cur, b.Xc, b.dots, k, n, D,
                           (long long)k * D, ksl, 0, tab);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_center_norms_kernel, dim3(k, S), dim3(64), 0, st, cur, b.shift_part + (size_t)S * k, b.st, D, k, force);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_assign_kernel, dim3((n + 63) / 64, S), dim3(1024), 0, st, b.dots, b.shift_part + (size_t)S * k, labels, b.st, tab, D, k, force, ksl);
        SQ_LAUNCH_CHECK();
        return members(force);
    };
    int it = 0;
    int done[2] = {0, 0};            // slides finished / of those, strictly converged (labels unchanged)
    while (it < max_iter) {
        const int burst = it == 0 ? 2 : 4;      // iterations between host checks of the done flags
        for (int q = 0; q < burst && it < max_iter; ++q, ++it) {
            if (int e = e_step(0)) return e;
            hipLaunchKernelGGL(km_sums_kernel, dim3(k, S), dim3(256), 0, st, b.Xc, b.members, b.offsets, b.sums, b.st, tab, D, k);
            SQ_LAUNCH_CHECK();
            hipLaunchKernelGGL(km_relocate_kernel, dim3(S), dim3(KM_THREADS), 0, st, b.Xc, cur, labels, b.offsets, b.sums,
                               b.weights, b.dist, b.st, tab, D, k);
            SQ_LAUNCH_CHECK();
            hipLaunchKernelGGL(km_update_centers_kernel, dim3(k, S), dim3(256), 0, st, cur, nxt, b.sums, b.weights, b.shift_part, b.st, D, k);
            SQ_LAUNCH_CHECK();
            hipLaunchKernelGGL(km_finish_iter_kernel, dim3(S), dim3(KM_THREADS), 0, st, b.shift_part, labels, b.labels_old, b.st, tab, k, max_iter);
            SQ_LAUNCH_CHECK();
            float* t = cur; cur = nxt; nxt = t;
        }
        hipLaunchKernelGGL(km_count_done_kernel, dim3(1), dim3(64), 0, st, b.st, S, b.done_count);
        SQ_LAUNCH_CHECK();
        SQ_HIP_CHECK(hipMemcpyAsync(done, b.done_count, 8, hipMemcpyDeviceToHost, st));
        SQ_HIP_CHECK(hipStreamSynchronize(st));
        if (done[0] == S) break;
    }
    // final E-step for the slides that did not converge strictly (labels must match the final centres).
    // For strictly converged slides the labels of the last E-step are already the answer and the
    // centres moved by a label-preserving update, so re-running the E-step for everyone is only
    // correct for the non-strict ones: the assign kernel is forced, then strict slides are restored.
    // When every slide converged strictly (the common case) nothing is left to do: labels and member lists are
    // those of the last E-step (_kmeans.py: the extra E-step runs only `if not strict_convergence`).
    if (!(done[0] == S && done[1] == S)) {
        // strict slides keep labels (== labels_old after the last update); non-strict get a fresh E-step
        if (int e = e_step(1)) return e;
        // restore labels of strict slides from labels_old and rebuild their member lists
        hipLaunchKernelGGL(km_restore_strict_kernel, dim3((n + 255) / 256, S), dim3(256), 0, st, labels, (const int*)b.labels_old, (const KmState*)b.st, tab);
        SQ_LAUNCH_CHECK();
        if (int e = members(1)) return e;
    }
    // the centres of the last update, centred coordinates (slides that stopped earlier were copied through every update)
    if (final_centers) SQ_HIP_CHECK(hipMemcpyAsync(final_centers, cur, (size_t)S * k * D * 4, hipMemcpyDeviceToDevice, st));
    if (cluster_features) {
        hipLaunchKernelGGL(km_cluster_means_kernel, dim3(k, S), dim3(256), 0, st, X, b.members, b.offsets, cluster_features, tab, D, k);
        SQ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(km_report_kernel, dim3((S + 63) / 64), dim3(64), 0, st, b.st, S, n_iter);
    SQ_LAUNCH_CHECK();
    return SQ_OK;
}

// ------------------------------------------------------------------------------------------
// 6. the driver behind the three entries
// ------------------------------------------------------------------------------------------
constexpr int KM_GRAM_MAX_N = 4096;              // the seeding kernel holds a slide's points in one workgroup's registers
constexpr int KM_RAGGED_MAX_SLIDES = 4096;

// What an entry refuses, in one order for all three: the sizes before the device pointers, so a caller can ask with
// NULL data why a shape is refused.  who: the entry's prefix; s_max: its bound on the slides (0: none); n_hi: on the
// rows of a slide.  shape_only: stop behind what the workspace size depends on.
int km_check(const char* who, const KmCounts& c, int s_max, int n_hi, int D, int k, bool shape_only, int trials, bool pointers) {
    if (s_max) SQ_REQUIRE(c.S >= 1 && c.S <= s_max, "%s: n_slides=%d, must be in 1..%d", who, c.S, s_max);
    else SQ_REQUIRE(c.S >= 1, "%s: n_slides=%d, must be at least 1", who, c.S);
    SQ_REQUIRE(c.ns && (shape_only || c.firsts), "%s: null pointer (n_samples / first_centers)", who);
    SQ_REQUIRE(k >= 1 && k <= KM_MAX_K, "%s: n_clusters=%d, must be in 1..%d", who, k, KM_MAX_K);
    const int distinct = c.stride ? c.S : 1;
    for (int s = 0; s < distinct; ++s)
        SQ_REQUIRE(c.n(s) >= k && c.n(s) <= n_hi, "%s: slide %d has n_samples=%d, must be in n_clusters=%d..%d%s", who, s, c.n(s), k, n_hi,
                   n_hi == KM_GRAM_MAX_N ? " (larger slides: sq_kmeans_fit_large)" : "");
    SQ_REQUIRE(D >= 4 && D % 4 == 0, "%s: dim=%d must be a multiple of 4", who, D);
    if (shape_only) return SQ_OK;
    SQ_REQUIRE(trials >= 1 && trials <= KM_MAX_TRIALS, "%s: n_local_trials=%d, must be in 1..%d", who, trials, KM_MAX_TRIALS);
    for (int s = 0; s < distinct; ++s)
        SQ_REQUIRE(c.first(s) >= 0 && c.first(s) < c.n(s), "%s: slide %d has first_center=%d outside 0..%d", who, s, c.first(s), c.n(s) - 1);
    SQ_REQUIRE(pointers, "%s: null pointer", who);
    return SQ_OK;
}

// The seeding from one fp64 Gram matrix per slide: every slide's seeds in b.seeds.
int km_seed_gram(const KmBufs& b, const KmExtents& e, int S, int D, int k, const double* uniforms, int trials, hipStream_t st) {
    const int n = e.n_max;
    hipLaunchKernelGGL(km_dgemm_nt_kernel, dim3((n + 63) / 64, (n + 63) / 64, S), dim3(256), 0, st, b.Xc, b.Xc, b.G, n, n, D, 0LL, 1, 1, b.tab);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_dist_f32_kernel, dim3(n, S), dim3(256), 0, st, b.G, b.dist32, b.tab);
    SQ_LAUNCH_CHECK();
    // one launch per class present: a slide's reduction layout depends on its own row count alone
    const int* list = b.cls_list;
    for (int q = 0; q < KM_SEED_CLASSES; list += e.cls_n[q++]) {
        if (!e.cls_n[q]) continue;
        const KmSeedLayout& lay = KM_SEED_LAYOUTS[q];
        hipLaunchKernelGGL(lay.pts == 2 ? km_seed_kernel<2> : km_seed_kernel<4>, dim3(e.cls_n[q]), dim3(lay.threads), 0, st, b.dist32, uniforms,
                           b.tab, list, k, trials, b.seeds);
        SQ_LAUNCH_CHECK();
    }
    return SQ_OK;
}

// The seeding of one slide of any size (section 5): its seeds in b.seeds.
int km_seed_large(const KmBufs& b, const KmLgBufs& lg, int n, int D, int k, int first_center, const double* uniforms, int trials,
                  hipStream_t st) {
    const int nchunks = (n + KM_LG_CHUNK - 1) / KM_LG_CHUNK, ntiles = (n + KM_LG_TILE - 1) / KM_LG_TILE;
    hipLaunchKernelGGL(km_lg_rows_kernel<0>, dim3(ntiles), dim3(256), 0, st, (const float*)b.Xc, lg.norms, (const int*)nullptr, (int*)nullptr,
                       (const float*)nullptr, (float*)nullptr, (double*)nullptr, n, D, 0, nchunks, 0, 0);
    SQ_LAUNCH_CHECK();
    // the first centre: closest = its distances, pot = their sum
    hipLaunchKernelGGL(km_lg_rows_kernel<1>, dim3(ntiles), dim3(256), 0, st, (const float*)b.Xc, lg.norms, (const int*)lg.cnt, lg.cand,
                       (const float*)lg.closest, lg.distc, lg.part, n, D, 1, nchunks, 1, first_center);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_lg_choose_kernel, dim3(nchunks), dim3(KM_LG_CHUNK), 0, st, (const double*)lg.part, (const float*)lg.distc,
                       (const int*)lg.cand, lg.closest, lg.chunk_sum, lg.pot, b.seeds, n, 1, ntiles, 1);
    SQ_LAUNCH_CHECK();
    for (int c = 1; c < k; ++c) {       // k - 1 dependent steps of three launches; the candidates never leave the device
        hipLaunchKernelGGL(km_lg_pick_kernel, dim3(nchunks), dim3(KM_LG_CHUNK), 0, st, (const float*)lg.closest, (const double*)lg.chunk_sum,
                           (const float*)lg.pot, uniforms + (size_t)(c - 1) * trials, lg.cnt, n, trials);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_lg_rows_kernel<1>, dim3(ntiles), dim3(256), 0, st, (const float*)b.Xc, lg.norms, (const int*)lg.cnt, lg.cand,
                           (const float*)lg.closest, lg.distc, lg.part, n, D, trials, nchunks, 0, 0);
        SQ_LAUNCH_CHECK();
        hipLaunchKernelGGL(km_lg_choose_kernel, dim3(nchunks), dim3(KM_LG_CHUNK), 0, st, (const double*)lg.part, (const float*)lg.distc,
                           (const int*)lg.cand, lg.closest, lg.chunk_sum, lg.pot, b.seeds + c, n, trials, ntiles, 0);
        SQ_LAUNCH_CHECK();
    }
    return SQ_OK;
}

// What sq_dbg_kmeans_lloyd puts in the place of the seeding: the centres the Lloyd loop starts from, where its last
// centres go, and which member lists it builds.
struct KmInject {
    const float* init_centers;        // f32 [S, k, D], centred coordinates
    float* final_centers;             // f32 [S, k, D] or nullptr
    bool large_lists;                 // the counting sort of section 5 (one slide) in place of km_members_kernel
};

// One fit: check, table, centring and tolerance, seeding (large: section 5 on the one slide, otherwise from the Gram
// matrices), then seeds -> centres and the Lloyd loop.  inj != nullptr: no seeding and no gather, the centres are given.
int km_fit(const char* who, int s_max, int n_hi, bool large, const float* X, const KmCounts& c, int D, int k, const double* uniforms,
           int trials, int max_iter, double tol, int32_t* labels, float* cluster_features, int32_t* seed_indices, int32_t* n_iter,
           void* workspace, size_t workspace_bytes, hipStream_t st, const KmInject* inj = nullptr) {
    if (int e = km_check(who, c, s_max, n_hi, D, k, false, trials, X && labels && (inj ? inj->init_centers != nullptr : uniforms != nullptr) && workspace))
        return e;
    if (inj && inj->large_lists) SQ_REQUIRE(c.S == 1, "%s: n_slides=%d, the large route's member lists take one slide", who, c.S);
    const int S = c.S;
    const bool lists = c.stride != 0;          // otherwise S equal slides: their table is filled on the device
    // The host block of a table made from lists must outlive its copy: the Lloyd loop synchronises the stream at its
    // first poll, every other way out waits here (`wait` is declared after `host`, so it runs first).
    std::vector<char> host;
    struct Wait {
        hipStream_t st;
        bool armed;
        ~Wait() { if (armed) (void)hipStreamSynchronize(st); }
    } wait{st, false};
    const KmExtents e = km_walk(c, lists ? &host : nullptr);
    KmBufs b;
    KmLgBufs lg;
    km_carve(S, e, D, k, (char*)workspace, &b, large ? &lg : nullptr);
    SQ_REQUIRE_WORKSPACE(who, workspace_bytes, b.bytes);
    if (lists) {
        wait.armed = true;
        SQ_HIP_CHECK(hipMemcpyAsync(b.tab, host.data(), host.size(), hipMemcpyHostToDevice, st));
    } else {
        hipLaunchKernelGGL(km_equal_table_kernel, dim3(1), dim3(256), 0, st, b.tab, b.cls_list, S, c.n(0), c.first(0), km_gram_elems(c.n(0)));
        SQ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(km_center_kernel, dim3((D + KC_COLS - 1) / KC_COLS, S), dim3(256), 0, st, X, b.Xc, b.colvar, b.tab, D);
    SQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_tol_kernel, dim3(S), dim3(256), 0, st, b.colvar, b.st, D, tol);
    SQ_LAUNCH_CHECK();
    const KmLgBufs* member_lists = large ? &lg : nullptr;
    if (inj) {
        SQ_HIP_CHECK(hipMemcpyAsync(b.centers, inj->init_centers, (size_t)S * k * D * 4, hipMemcpyDeviceToDevice, st));
        if (inj->large_lists) {
            // Only the per-chunk histograms of section 5 are needed, and the Gram matrix is not: they lie in its place.
            // ((nchunks - 1) * 256 + k) ints against n^2 doubles: k <= n covers one chunk, n > 1024 any number of them.
            lg = KmLgBufs{};
            lg.hist = (int*)b.G;
            member_lists = &lg;
        }
    } else {
        if (int rc = large ? km_seed_large(b, lg, e.n_max, D, k, c.first(0), uniforms, trials, st) : km_seed_gram(b, e, S, D, k, uniforms, trials, st))
            return rc;
        if (seed_indices) SQ_HIP_CHECK(hipMemcpyAsync(seed_indices, b.seeds, (size_t)S * k * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(km_gather_centers_kernel, dim3(k, S), dim3(256), 0, st, b.Xc, b.seeds, b.centers, b.tab, D, k);
        SQ_LAUNCH_CHECK();
    }
    SQ_HIP_CHECK(hipMemsetAsync(b.labels_old, 0xff, e.rows * 4, st));          // labels_old = -1
    const int rc = km_lloyd_and_means(X, S, e.n_max, D, k, max_iter, labels, cluster_features, n_iter, inj ? inj->final_centers : nullptr, b,
                                      member_lists, st);
    wait.armed = lists && (rc != SQ_OK || max_iter < 1);          // no poll ran
    return rc;
}

size_t km_workspace(const KmCounts& c, int D, int k, bool large) {
    KmBufs b;
    KmLgBufs lg;
    km_carve(c.S, km_walk(c, nullptr), D, k, nullptr, &b, large ? &lg : nullptr);
    return b.bytes;
}

}  // namespace

extern "C" size_t sq_kmeans_workspace_bytes(int n_slides, int n_samples, int dim, int n_clusters) {
    if (n_slides < 1 || n_samples < 1 || dim < 1 || n_clusters < 1) return 0;
    return km_workspace(KmCounts{n_slides, &n_samples, nullptr, 0}, dim, n_clusters, false);
}

extern "C" size_t sq_kmeans_large_workspace_bytes(int n_samples, int dim, int n_clusters) {
    if (n_samples < 1 || n_samples > KM_LG_MAX_N || dim < 1 || n_clusters < 1) return 0;
    return km_workspace(KmCounts{1, &n_samples, nullptr, 0}, dim, n_clusters, true);
}

extern "C" size_t sq_kmeans_ragged_workspace_bytes(int n_slides, const int32_t* n_samples, int dim, int n_clusters) {
    const KmCounts c{n_slides, n_samples, nullptr, 1};
    if (km_check("kmeans (ragged)", c, KM_RAGGED_MAX_SLIDES, KM_GRAM_MAX_N, dim, n_clusters, true, 0, false) != SQ_OK) return 0;
    return km_workspace(c, dim, n_clusters, false);
}

extern "C" int sq_kmeans_fit(const float* X, int S, int n, int D, int k, int first_center, const double* uniforms,
                             int n_local_trials, int max_iter, double tol, int32_t* labels, float* cluster_features,
                             int32_t* seed_indices, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                             sq_stream_t stream) {
    return km_fit("kmeans", 0, KM_GRAM_MAX_N, false, X, KmCounts{S, &n, &first_center, 0}, D, k, uniforms, n_local_trials, max_iter, tol,
                  labels, cluster_features, seed_indices, n_iter, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int sq_kmeans_fit_large(const float* X, int n, int D, int k, int first_center, const double* uniforms,
                                   int n_local_trials, int max_iter, double tol, int32_t* labels, float* cluster_features,
                                   int32_t* seed_indices, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                                   sq_stream_t stream) {
    return km_fit("kmeans (large)", 0, KM_LG_MAX_N, true, X, KmCounts{1, &n, &first_center, 0}, D, k, uniforms, n_local_trials, max_iter, tol,
                  labels, cluster_features, seed_indices, n_iter, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int sq_kmeans_fit_ragged(const float* X, int S, const int32_t* n_samples, int D, int k, const int32_t* first_centers,
                                    const double* uniforms, int n_local_trials, int max_iter, double tol, int32_t* labels,
                                    float* cluster_features, int32_t* seed_indices, int32_t* n_iter, void* workspace,
                                    size_t workspace_bytes, sq_stream_t stream) {
    return km_fit("kmeans (ragged)", KM_RAGGED_MAX_SLIDES, KM_GRAM_MAX_N, false, X, KmCounts{S, n_samples, first_centers, 1}, D, k, uniforms,
                  n_local_trials, max_iter, tol, labels, cluster_features, seed_indices, n_iter, workspace, workspace_bytes,
                  (hipStream_t)stream);
}

// Test hook: sq_kmeans_fit with the seeding and the centre gather replaced by given centres (see the header).
extern "C" int sq_dbg_kmeans_lloyd(const float* X, int S, int n, int D, int k, const float* init_centers, int large_lists, int max_iter,
                                   double tol, int32_t* labels, float* cluster_features, float* final_centers, int32_t* n_iter,
                                   void* workspace, size_t workspace_bytes, sq_stream_t stream) {
    const int first_center = 0;
    const KmInject inj{init_centers, final_centers, large_lists != 0};
    return km_fit("kmeans (dbg lloyd)", 0, KM_GRAM_MAX_N, false, X, KmCounts{S, &n, &first_center, 0}, D, k, nullptr, 1, max_iter, tol, labels,
                  cluster_features, nullptr, n_iter, workspace, workspace_bytes, (hipStream_t)stream, &inj);
}
